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
refuses, with the block's name, anything the kernels do not serve.  Off by default (teacher_runner.VGGTTeacherRunner(fused_blocks=True)).

All three stacks are pre-norm ViT blocks: one pack (_ViTBlock, read through teacher_read.Reader) and one body (self_attn, mlp, block) serve
them; what differs between them is what stands between the QKV GEMM and attention, and the decoder's cross-attention middle."""
import torch

from . import ops
from . import teacher_glue as tg
from ._lib import GdHipError
from .teacher_read import Reader, f32


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


def _attention(r, attn, C, what, rope):
    """-> (H, RoPE base) of an attention module the kernels serve: head dim 64, scale 64^-0.5, a RoPE module exactly when `rope`."""
    H = int(r.need(attn, "num_heads", what))
    if C % H or C // H != 64:
        r.fail(f"{what}.num_heads", f"head dim {C / H:g} (width {C}, {H} heads): the attention kernels serve head dim 64")
    scale = float(getattr(attn, "scale", 64 ** -0.5))
    if abs(scale - 64 ** -0.5) > 1e-9:
        r.fail(f"{what}.scale", f"{scale} is not 64^-0.5")
    m = getattr(attn, "rope", None)
    if rope and m is None:            # (named as '<what>.rope is None' after the attention module's path: the wording the GPU tests of CroCo look for)
        r.fail(what, f"{what}.rope is None: the fused q / k step always rotates")
    if not rope and m is not None:
        r.fail(f"{what}.rope", f"{type(m).__name__}: these blocks run without a rotary step")
    return H, float(getattr(m, "base_frequency", getattr(m, "base", 100.0)))


def _qk_norms(r, attn, qk):
    """-> ((q gamma, q beta, k gamma, k beta), eps) as gd_qk_norm_rope takes them: four None and 0.0 where q and k are not normed."""
    plain = (None, None, None, None), 0.0
    if qk == "rope":
        return plain
    qn, kn = r.need(attn, "q_norm", "attn"), r.need(attn, "k_norm", "attn")
    if all(isinstance(m, torch.nn.Identity) for m in (qn, kn)):
        return plain
    are = f"{type(qn).__name__} with k_norm {type(kn).__name__}"
    if qk is None:
        r.fail("attn.q_norm", f"{are}: served is Identity on both")
    if not all(isinstance(m, torch.nn.LayerNorm) for m in (qn, kn)):
        r.fail("attn.q_norm", f"{are}: served are LayerNorm(64) with affine on both, or Identity on both")
    (gq, bq, eps), (gk, bk, eps_k) = r.ln(qn, "attn.q_norm", 64), r.ln(kn, "attn.k_norm", 64)
    if eps != eps_k:
        r.fail("attn.q_norm", "differs from attn.k_norm in eps")
    return (gq, bq, gk, bk), eps


class _ViTBlock:
    """One pre-norm ViT block's tensors in the form the kernels take: matrices in the operand dtype, vectors in fp32; LayerScale, where the block
    has one, folded into proj / fc2.
    qk: what stands between the QKV GEMM and attention — "norm+rope" (the aggregator: q_norm / k_norm LayerNorm(64) on both or Identity on both,
    then RoPE), "rope" (CroCo: RoPE alone, no q / k norm in the module) or None (DINOv2: neither; both norms Identity, no rope module).
    cross: a CroCo decoder block — also `cross_attn` (projq, projk | projv as one [2C, C] matrix, proj), `norm2` in front of it, `norm_y`
    (LayerNorm, or Identity with norm_mem=False: ny = None), and the MLP's norm is `norm3`."""

    def __init__(self, r, blk, dtype, qk, cross=False):
        op = lambda t: t.detach().to(dtype).contiguous()
        attn, mlp = r.need(blk, "attn"), r.need(blk, "mlp")
        qkv = r.need(attn, "qkv", "attn")
        C = self.C = qkv.weight.shape[1]
        self.rotary = qk is not None
        self.H, self.base = _attention(r, attn, C, "attn", self.rotary)
        self.qk, self.qk_eps = _qk_norms(r, attn, qk)
        r.exact_gelu(getattr(mlp, "act", None), "mlp.act", allow_none=True)
        self.n1 = r.ln(r.need(blk, "norm1"), "norm1", C)
        nmlp = "norm3" if cross else "norm2"
        self.nmlp = r.ln(r.need(blk, nmlp), nmlp, C)
        self.wqkv, self.bqkv = op(qkv.weight), f32(qkv.bias)
        wp, bp = fold_layer_scale(r.need(attn, "proj", "attn"), getattr(blk, "ls1", None))
        self.wproj, self.bproj = op(wp), f32(bp)
        fc1 = r.need(mlp, "fc1", "mlp")
        self.w1, self.b1 = op(fc1.weight), f32(fc1.bias)
        w2, b2 = fold_layer_scale(r.need(mlp, "fc2", "mlp"), getattr(blk, "ls2", None))
        self.w2, self.b2 = op(w2), f32(b2)
        if not cross:
            return
        ca = r.need(blk, "cross_attn")
        pq, pk, pv, po = (r.need(ca, a, "cross_attn") for a in ("projq", "projk", "projv", "proj"))
        Hc, base_c = _attention(r, ca, C, "cross_attn", True)
        if (Hc, base_c) != (self.H, self.base):
            r.fail("cross_attn", f"differs from attn in heads / RoPE base ({Hc}, {base_c:g} against {self.H}, {self.base:g})")
        if (pk.bias is None) != (pv.bias is None):
            r.fail("cross_attn.projk", "one of projk and projv has a bias, the other has none")
        self.n2 = r.ln(r.need(blk, "norm2"), "norm2", C)
        ny = r.need(blk, "norm_y")
        self.ny = None if isinstance(ny, torch.nn.Identity) else r.ln(ny, "norm_y", C)
        self.wq, self.bq = op(pq.weight), f32(pq.bias)
        # k and v projections of the other view's tokens as ONE GEMM: kv [M, 2C] = [projk | projv], the layout gd_cross_attention_fwd reads
        self.wkv = op(torch.cat([pk.weight.detach(), pv.weight.detach()], dim=0))
        self.bkv = None if pk.bias is None else f32(torch.cat([pk.bias.detach(), pv.bias.detach()]))
        self.wcproj, self.bcproj = op(po.weight), f32(po.bias)


def _blocks(who, prefix, blocks, dtype, qk, cross=False):
    return [_ViTBlock(Reader(who, f"{prefix}[{i}]"), b, dtype, qk, cross) for i, b in enumerate(blocks)]


def _operand_dtype(who, dtype):
    if dtype not in (torch.float32, torch.bfloat16):
        raise GdHipError(f"{who}: dtype must be torch.float32 or torch.bfloat16")
    return dtype


def self_attn(p, x, pos, B, N, dtype, want_qk=False):
    """x [B*N, C] fp32 residual stream -> (x + proj(attention(norm1(x))) fp32, the (q, k) qk_norm_rope hands out with want_qk, else None)."""
    y, _, _ = ops.layernorm_fwd(x, *p.n1, save_stats=False, out_dtype=dtype)
    qkv = ops.gemm_nt(y, p.wqkv, bias=p.bqkv)
    # in place on qkv; null gamma / beta (CroCo, an Identity-normed aggregator block): plain RoPE of q and k.  Without a rotary step
    # attention_fwd reads the packed qkv as the GEMM wrote it.
    qk = ops.qk_norm_rope(qkv, B, N, p.H, pos, *p.qk, p.qk_eps, p.base, want_qk=want_qk) if p.rotary else None
    o, _ = ops.attention_fwd(qkv, B, N, p.H)
    return ops.gemm_nt(o, p.wproj, out_dtype=torch.float32, bias=p.bproj, residual=x), qk


def mlp(p, x, dtype):
    y, _, _ = ops.layernorm_fwd(x, *p.nmlp, save_stats=False, out_dtype=dtype)
    h = ops.gemm_nt(y, p.w1, bias=p.b1, act=1)
    return ops.gemm_nt(h, p.w2, out_dtype=torch.float32, bias=p.b2, residual=x)


def block(p, x, pos, B, N, dtype, want_qk=False):
    """x [B*N, C] fp32 residual stream -> (x after the block, (q, k) or None)."""
    x, qk = self_attn(p, x, pos, B, N, dtype, want_qk)
    return mlp(p, x, dtype), qk


class FusedAggregatorBlocks:
    """FusedAggregatorBlocks(aggregator, dtype=torch.bfloat16).forward(tokens, pos, B, S) -> (outputs, maps).

    dtype: the operand type of the matrix products and of attention.  torch.bfloat16: bf16 operands, fp32 accumulation, and the residual
    stream kept in fp32 (as autocast keeps it): LayerNorm reads fp32 and writes the bf16 operand, the proj / fc2 GEMMs add the fp32
    residual and write fp32.  torch.float32: everything exact fp32, the parity mode."""

    def __init__(self, aggregator, dtype=torch.bfloat16):
        who, r = "FusedAggregatorBlocks", Reader("FusedAggregatorBlocks", "aggregator")
        self.dtype = _operand_dtype(who, dtype)
        frame, glob = r.need(aggregator, "frame_blocks"), r.need(aggregator, "global_blocks")
        order = list(getattr(aggregator, "aa_order", ["frame", "global"]))
        if order != ["frame", "global"]:
            r.fail("aa_order", f"{order}: served is ['frame', 'global']")
        self.per = int(getattr(aggregator, "aa_block_size", 1))
        depth = len(frame)
        if len(glob) != depth or depth % self.per:
            r.fail("frame_blocks", f"{depth} frame / {len(glob)} global blocks do not pair up in groups of {self.per}")
        # aggregator.py:255-260 keeps the map of iteration i `if i in self.attn_indices`: an index past the last iteration never matches
        self.attn_indices = sorted({int(i) for i in (getattr(aggregator, "attn_indices", None) or []) if 0 <= int(i) < depth // self.per})
        self.temperature = float(getattr(aggregator, "temperature", 1.0))
        self.prefix = int(r.need(aggregator, "patch_start_idx"))
        self.frame = _blocks(who, "frame_blocks", frame, dtype, "norm+rope")
        self.glob = _blocks(who, "global_blocks", glob, dtype, "norm+rope")

    def _block(self, p, x, pos, B, N, want_qk=False):
        """One block alone (what the per-block tests call; `forward` calls `block` itself)."""
        return block(p, x, pos, B, N, self.dtype, want_qk)

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
                x, _ = block(self.frame[j], x, pos, BS, P, self.dtype)
                inter.append(x)
            for k, j in enumerate(range(it * self.per, (it + 1) * self.per)):
                x, qk = block(self.glob[j], x, pos, B, S * P, self.dtype, j in sel)
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
        who, r = self.WHO, Reader(self.WHO, name)
        fail, need = r.fail, r.need
        _operand_dtype(who, dtype)
        blocks = getattr(embedder, "blocks", None)
        if blocks is None:
            fail("blocks", "missing (the 'conv' patch embedder is one convolution: leave fused_patch_embed off)")
        if getattr(embedder, "chunked_blocks", False):
            fail("chunked_blocks", "true: served is a flat block list (block_chunks=0)")
        D = int(need(embedder, "pos_embed").shape[-1])
        if D % 8 or D > 2048:
            fail("pos_embed", f"width {D}: served is a multiple of 8 up to 2048")
        P = need(embedder, "patch_size")
        P = int(P[0] if isinstance(P, (tuple, list)) else P)
        pe = need(embedder, "patch_embed")
        proj = need(pe, "proj", "patch_embed")
        if not (isinstance(proj, torch.nn.Conv2d) and tuple(proj.kernel_size) == (P, P) and tuple(proj.stride) == (P, P) and
                tuple(proj.padding) == (0, 0) and tuple(proj.dilation) == (1, 1) and proj.groups == 1 and proj.in_channels == 3 and
                proj.out_channels == D):
            fail("patch_embed.proj", f"{proj}: served is Conv2d(3, {D}, kernel_size={P}, stride={P})")
        if not isinstance(getattr(pe, "norm", None), (torch.nn.Identity, type(None))):
            fail("patch_embed.norm", f"{type(pe.norm).__name__}: served is Identity")
        R = int(need(embedder, "num_register_tokens"))
        reg = getattr(embedder, "register_tokens", None)
        if (0 if reg is None else int(reg.shape[-2])) != R or (reg is not None and int(reg.shape[-1]) != D):
            fail("register_tokens", f"{None if reg is None else tuple(reg.shape)} disagrees with num_register_tokens = {R} at width {D}")
        cls = need(embedder, "cls_token")
        if cls.numel() != D:
            fail("cls_token", f"{tuple(cls.shape)} is not one token of width {D}")
        if not callable(getattr(embedder, "interpolate_pos_encoding", None)):
            fail("interpolate_pos_encoding", "missing")
        self.norm = r.ln(need(embedder, "norm"), "norm", D)
        self.blocks = _blocks(who, f"{name}.blocks", blocks, dtype, None)
        for i, p in enumerate(self.blocks):
            if p.C != D:
                fail(f"blocks[{i}].attn.qkv", f"width {p.C} is not the embedder's {D}")
        self.embedder, self.name, self.dtype, self.D, self.P, self.R = embedder, name, dtype, D, P, R
        K = 3 * P * P
        self.Kp = (K + 63) // 64 * 64                                 # the patch convolution as a [D, Kp] matrix (vit.GDViT._patch_plan)
        wp = torch.zeros(D, self.Kp, dtype=torch.float32, device=proj.weight.device)
        wp[:, :K] = proj.weight.detach().float().reshape(D, K)
        self.wpe, self.bpe = wp.to(dtype).contiguous(), f32(proj.bias)
        self.cls = f32(cls).reshape(D)
        self.reg = None if reg is None else f32(reg).reshape(R, D)
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
            x, _ = block(p, x, None, BS, Nt, self.dtype)
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
        r = Reader(self.WHO, "aggregator")
        cam, reg, prefix, _, _ = (r.need(aggregator, a) for a in ("camera_token", "register_token", "patch_start_idx", "_resnet_mean", "_resnet_std"))
        prefix = int(prefix)
        if prefix < 1:
            r.fail("patch_start_idx", f"{prefix}: served is a camera token (and registers) in front of the patches")
        if cam.shape[-1] != self.D or tuple(cam.shape[:3]) != (1, 2, 1):
            r.fail("camera_token", f"{tuple(cam.shape)}: the embedder's width is {self.D} (expected [1, 2, 1, {self.D}])")
        if tuple(reg.shape) != (1, 2, prefix - 1, self.D):
            r.fail("register_token", f"{tuple(reg.shape)} does not fit patch_start_idx = {prefix} at width {self.D}")
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
        r = Reader(_WHO, "matcher")
        self.dtype = _operand_dtype(_WHO, dtype)
        enc, de, dec1, dec2, dnorm = (r.need(matcher, a) for a in ("enc_blocks", "decoder_embed", "dec_blocks", "dec_blocks2", "dec_norm"))
        if len(dec1) != len(dec2):
            r.fail("dec_blocks", f"{len(dec1)} blocks and the {len(dec2)} of dec_blocks2 differ in length")
        if len(dec1) == 0:
            r.fail("dec_blocks", "empty")
        self.enc = _blocks(_WHO, "enc_blocks", enc, dtype, "rope")
        self.dec1 = _blocks(_WHO, "dec_blocks", dec1, dtype, "rope", cross=True)
        self.dec2 = _blocks(_WHO, "dec_blocks2", dec2, dtype, "rope", cross=True)
        self.wde, self.bde = r.linear(de, "decoder_embed", cast=lambda t: t.detach().to(dtype).contiguous())
        Cd = self.wde.shape[0]
        for nm, stack in (("dec_blocks", self.dec1), ("dec_blocks2", self.dec2)):
            for i, p in enumerate(stack):
                if p.C != Cd:
                    Reader(_WHO, f"{nm}[{i}]").fail("attn.qkv", f"width {p.C} is not decoder_embed's {Cd}")
        self.dnorm = r.ln(dnorm, "dec_norm", Cd)

    # -- pieces ---------------------------------------------------------------------------------------------------------------------
    def _enc_block(self, p, x, pos, B, N):
        """x [B*N, C] fp32 residual stream -> the same after one encoder block (what the per-block tests call; `encode` calls `block` itself)."""
        return block(p, x, pos, B, N, self.dtype)[0]

    def _dec_block(self, p, x, y, xpos, ypos, B, Nx, Ny):
        """x [B*Nx, C], y [B*Ny, C] fp32 (this view's tokens, the other view's: read only) -> (x after the block, camap [B, 1, Nx, Ny] fp32:
        the head mean of the raw scaled scores)."""
        from .rope import rope_2d
        dt, C, H = self.dtype, p.C, p.H
        x, _ = self_attn(p, x, xpos, B, Nx, dt)
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
        return mlp(p, x, dt), camap.unsqueeze(1)

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
            t, _ = block(p, t, p2, B, N, self.dtype)
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
