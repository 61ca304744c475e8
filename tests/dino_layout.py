"""A module tree with the layout and attribute names of the VGGT teacher's DINOv2 patch embedder (vggt/layers/vision_transformer.py: `patch_embed.proj`,
`cls_token`, `register_tokens`, `pos_embed`, `mask_token`, `blocks[i].{norm1, attn.{qkv, proj, q_norm, k_norm, rope}, ls1, norm2, mlp.{fc1, act, fc2}, ls2}`,
`norm`, `interpolate_pos_encoding`), and an aggregator layout around it whose forward takes the embedder's dict (vggt/models/aggregator.py:216-219).
Filled by `fill_params` of tests/test_teacher_runner_ref.py; fixture G29 (tools/make_golden_g29.py) holds what the reference's own classes returned with
the same weights.  A test helper, not a test module."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from test_teacher_runner_ref import AggregatorLayout, _LayerScale, _PatchEmbed

DINO_CFG = dict(img_size=56, patch_size=14, embed_dim=128, depth=3, num_heads=2, num_register_tokens=4)
DINO_SIZES = [(56, 56), (42, 70), (70, 42), (28, 28)]          # the table's own grid; non-square both ways; square and resampled
AGG_CFG = dict(img_size=56, patch_size=14, embed_dim=384, depth=2, num_heads=6, num_register_tokens=4, attn_indices=[0, 1], temperature=1.0)
AGG_DINO = dict(depth=12, num_heads=6)                         # dinov2_vits14_reg


def param_layout(module):
    return ",".join(f"{n}:{'x'.join(map(str, p.shape))}" for n, p in sorted(module.named_parameters()))


class _DinoAttention(nn.Module):
    """Plain multi-head attention: no q/k norm (Identity), no rotary step.  `sdpa`: the product through F.scaled_dot_product_attention (the reference's
    MemEffAttention with xformers installed runs a memory-efficient kernel; without it, the explicit softmax below)."""
    sdpa = False

    def __init__(self, dim, heads):
        super().__init__()
        self.num_heads, self.head_dim = heads, dim // heads
        self.scale = self.head_dim ** -0.5
        self.qkv, self.proj = nn.Linear(dim, 3 * dim), nn.Linear(dim, dim)
        self.q_norm, self.k_norm, self.rope = nn.Identity(), nn.Identity(), None

    def forward(self, x):
        B, N, C = x.shape
        q, k, v = self.qkv(x).reshape(B, N, 3, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4).unbind(0)
        if self.sdpa:
            o = F.scaled_dot_product_attention(q, k, v)                                  # scale = head_dim ** -0.5 = self.scale
        else:
            o = F.softmax((q * self.scale) @ k.transpose(-2, -1), dim=-1) @ v
        return self.proj(o.transpose(1, 2).reshape(B, N, C))


class _DinoMlp(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.fc1, self.act, self.fc2 = nn.Linear(dim, 4 * dim), nn.GELU(), nn.Linear(4 * dim, dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class _DinoBlock(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.norm1, self.norm2 = nn.LayerNorm(dim, eps=1e-6), nn.LayerNorm(dim, eps=1e-6)
        self.attn, self.mlp = _DinoAttention(dim, heads), _DinoMlp(dim)
        self.ls1, self.ls2 = _LayerScale(dim), _LayerScale(dim)

    def forward(self, x):
        x = x + self.ls1(self.attn(self.norm1(x)))
        return x + self.ls2(self.mlp(self.norm2(x)))


class DinoLayout(nn.Module):
    """forward(img [BS, 3, H, W], already normalised) -> the embedder's dict.  The position table is resampled as the teacher's configuration does
    (aggregator.py:157-160: bicubic, antialias, no offset: an output SIZE, not a scale factor)."""

    def __init__(self, img_size, patch_size, embed_dim, depth, num_heads, num_register_tokens):
        super().__init__()
        self.patch_size, self.num_register_tokens, self.chunked_blocks = patch_size, num_register_tokens, False
        self.patch_embed = _PatchEmbed(patch_size, embed_dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, (img_size // patch_size) ** 2 + 1, embed_dim))
        self.register_tokens = nn.Parameter(torch.zeros(1, num_register_tokens, embed_dim)) if num_register_tokens else None
        self.mask_token = nn.Parameter(torch.zeros(1, embed_dim))          # unused without masks; a parameter of the reference, so `fill_params` must see it
        self.blocks = nn.ModuleList([_DinoBlock(embed_dim, num_heads) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=1e-6)

    def interpolate_pos_encoding(self, x, w, h):
        """(tokens [., 1 + Np, D], w = the image's first spatial extent, h = its second) -> [1, 1 + Np, D]."""
        N = self.pos_embed.shape[1] - 1
        if x.shape[1] - 1 == N and w == h:
            return self.pos_embed
        pe = self.pos_embed.float()
        M = math.isqrt(N)
        grid = F.interpolate(pe[:, 1:].reshape(1, M, M, -1).permute(0, 3, 1, 2), size=(w // self.patch_size, h // self.patch_size), mode="bicubic",
                             antialias=True)
        return torch.cat([pe[:, :1], grid.permute(0, 2, 3, 1).reshape(1, -1, pe.shape[-1])], dim=1).to(x.dtype)

    def forward(self, img, masks=None):
        assert masks is None
        BS, _, H, W = img.shape
        x = torch.cat([self.cls_token.expand(BS, -1, -1), self.patch_embed(img)], dim=1)
        x = x + self.interpolate_pos_encoding(x, H, W)
        if self.register_tokens is not None:
            x = torch.cat([x[:, :1], self.register_tokens.expand(BS, -1, -1), x[:, 1:]], dim=1)
        for blk in self.blocks:
            x = blk(x)
        xn, R = self.norm(x), self.num_register_tokens
        return {"x_norm_clstoken": xn[:, 0], "x_norm_regtokens": xn[:, 1:R + 1], "x_norm_patchtokens": xn[:, R + 1:], "x_prenorm": x, "masks": masks}


class _TakePatchTokens(nn.Module):
    """What aggregator.py:218-219 does with the embedder's return: a dict gives its `x_norm_patchtokens`."""

    def __init__(self, embedder):
        super().__init__()
        self.embedder = [embedder]           # not registered: the parameters stay under the aggregator's `patch_embed`

    def forward(self, x):
        out = self.embedder[0](x)
        return out["x_norm_patchtokens"] if isinstance(out, dict) else out


class DinoAggregatorLayout(AggregatorLayout):
    """AggregatorLayout with the DINO layout as its `patch_embed` and the reference's buffer names (`_resnet_mean`, `_resnet_std`).  `forward` is the
    parent's: for its duration `patch_embed` answers with the patch tokens of the embedder's dict."""

    def __init__(self, img_size, patch_size, embed_dim, depth, num_heads, num_register_tokens, attn_indices, temperature, dino_depth, dino_heads):
        super().__init__(img_size, patch_size, embed_dim, depth, num_heads, num_register_tokens, attn_indices, temperature)
        self.patch_embed = DinoLayout(img_size, patch_size, embed_dim, dino_depth, dino_heads, num_register_tokens)
        self.register_buffer("_resnet_mean", self.mean.clone(), persistent=False)
        self.register_buffer("_resnet_std", self.std.clone(), persistent=False)

    def forward(self, images):
        embedder = self.patch_embed
        self._modules["patch_embed"] = _TakePatchTokens(embedder)
        try:
            return super().forward(images)
        finally:
            self._modules["patch_embed"] = embedder
