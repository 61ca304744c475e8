"""The VGGT teacher's alternating-attention stack (vggt/models/aggregator.py:246-275: `aa_block_size` frame blocks on [B*S, P], then
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

    def __init__(self, blk, name, dtype):
        def need(obj, attr, where):
            if not hasattr(obj, attr):
                raise GdHipError(f"FusedAggregatorBlocks: {name}: {where} has no `{attr}`")
            return getattr(obj, attr)
        attn, mlp = need(blk, "attn", "the block"), need(blk, "mlp", "the block")
        H = int(need(attn, "num_heads", "attn"))
        C = need(attn, "qkv", "attn").weight.shape[1]
        if C % H or C // H != 64:
            raise GdHipError(f"FusedAggregatorBlocks: {name}: head dim {C / H:g} (width {C}, {H} heads): the attention kernels serve head dim 64")
        scale = float(getattr(attn, "scale", 64 ** -0.5))
        if abs(scale - 64 ** -0.5) > 1e-9:
            raise GdHipError(f"FusedAggregatorBlocks: {name}: attn.scale {scale} is not 64^-0.5")
        qn, kn = need(attn, "q_norm", "attn"), need(attn, "k_norm", "attn")
        ln = [isinstance(m, torch.nn.LayerNorm) and m.elementwise_affine and tuple(m.normalized_shape) == (64,) for m in (qn, kn)]
        ident = [isinstance(m, torch.nn.Identity) for m in (qn, kn)]
        if not (all(ln) or all(ident)):
            raise GdHipError(f"FusedAggregatorBlocks: {name}: q_norm / k_norm are {type(qn).__name__} / {type(kn).__name__}: served are "
                             "LayerNorm(64) with affine on both, or Identity on both")
        if all(ln) and qn.eps != kn.eps:
            raise GdHipError(f"FusedAggregatorBlocks: {name}: q_norm and k_norm differ in eps")
        rope = getattr(attn, "rope", None)
        if rope is None:
            raise GdHipError(f"FusedAggregatorBlocks: {name}: attn.rope is None: the fused q/k step always rotates")
        act = getattr(mlp, "act", None)           # vggt/layers/mlp.py: act_layer(); a layout without the attribute calls F.gelu itself
        if act is not None and not (isinstance(act, torch.nn.GELU) and getattr(act, "approximate", "none") == "none"):
            raise GdHipError(f"FusedAggregatorBlocks: {name}: mlp.act is {act}: the GEMM epilogue serves exact (erf) GELU")
        for nm in ("norm1", "norm2"):
            m = need(blk, nm, "the block")
            if not (isinstance(m, torch.nn.LayerNorm) and m.elementwise_affine and tuple(m.normalized_shape) == (C,)):
                raise GdHipError(f"FusedAggregatorBlocks: {name}: {nm} is not an affine LayerNorm({C})")
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
