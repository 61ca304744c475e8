"""CPU: the teacher runner's hooks against the REFERENCE's VGGT aggregator (vggt/models/aggregator.py, tiny configuration), through fixture G22.
G22 (tools/make_golden_g22.py) holds what the reference's own Aggregator returned on one image pair with the deterministic weights of
`fill_params`: its token outputs and its `attn_mean`.  The test runs a module tree with the aggregator's layout (same parameter names, one RoPE
module shared by every block, q/k-norm on, global blocks called with return_attn=True) that must reproduce those outputs, and then checks:
  * QKCapture picks up exactly the q / k the selected global blocks multiply: rebuilding the cross-view maps from them (oracle formula = what
    gd_cross_view_attn computes on the GPU, tests/test_gpu_teacher_glue.py) reproduces the reference's `attn_mean`;
  * under `_no_attention_maps` the aggregator's token outputs are unchanged while no [B, H, n, n] map is formed."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

import gd_oracle as O

CFG = dict(img_size=56, patch_size=14, embed_dim=128, depth=3, num_heads=2, num_register_tokens=4, attn_indices=[1, 2], temperature=0.8)


def fill_params(module, seed=22):
    """Deterministic weights by parameter name (the fixture's generator fills the reference's Aggregator the same way): matrices and tokens
    N(0, 1 / fan-in), LayerNorm weights and LayerScale gammas 1 + N(0, 0.1^2), biases N(0, 0.1^2)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in sorted(module.named_parameters()):
            r = torch.randn(p.shape, generator=g, dtype=torch.float32)
            if p.ndim >= 2:
                p.copy_(r / math.sqrt(p[0].numel()))
            else:
                p.copy_((1.0 if name.endswith(("weight", "gamma")) else 0.0) + 0.1 * r)


class _Rope2D(nn.Module):
    """2-D RoPE on [B, H, N, D] (oracle.rope_2d holds the arithmetic; one instance is shared by every block, as in the aggregator)."""

    def forward(self, tokens, positions):
        return O.rope_2d(tokens.transpose(1, 2), positions).transpose(1, 2)


class _Attention(nn.Module):
    def __init__(self, dim, heads, rope):
        super().__init__()
        self.num_heads, self.head_dim = heads, dim // heads
        self.scale = self.head_dim ** -0.5
        self.qkv = nn.Linear(dim, 3 * dim)
        self.q_norm, self.k_norm = nn.LayerNorm(self.head_dim), nn.LayerNorm(self.head_dim)
        self.proj = nn.Linear(dim, dim)
        self.rope = rope

    def forward(self, x, pos=None, return_attn=False, temperature=1.0):
        B, N, C = x.shape
        q, k, v = self.qkv(x).reshape(B, N, 3, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4).unbind(0)
        q, k = self.q_norm(q), self.k_norm(k)
        q, k = self.rope(q, pos), self.rope(k, pos)
        q = q * self.scale
        out = self.proj((F.softmax(q @ k.transpose(-2, -1), dim=-1) @ v).transpose(1, 2).reshape(B, N, C))
        if not return_attn:
            return out
        n = N // 2                      # two views, 5 prefix tokens each: view-1 patches against view-2 patches and back
        m1 = F.softmax(q[..., 5:n, :] @ k[..., n + 5:, :].transpose(-2, -1) / temperature, dim=-1)
        m2 = F.softmax(q[..., n + 5:, :] @ k[..., 5:n, :].transpose(-2, -1) / temperature, dim=-1)
        return out, torch.cat([m1, m2], dim=0)


class _LayerScale(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(dim))

    def forward(self, x):
        return x * self.gamma


class _Mlp(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(dim, 4 * dim), nn.Linear(4 * dim, dim)

    def forward(self, x):
        return self.fc2(F.gelu(self.fc1(x)))


class _Block(nn.Module):
    def __init__(self, dim, heads, rope):
        super().__init__()
        self.norm1, self.norm2 = nn.LayerNorm(dim), nn.LayerNorm(dim)
        self.attn = _Attention(dim, heads, rope)
        self.ls1, self.ls2 = _LayerScale(dim), _LayerScale(dim)
        self.mlp = _Mlp(dim)

    def forward(self, x, pos=None, return_attn=False, temperature=1.0):
        if return_attn:
            a, maps = self.attn(self.norm1(x), pos=pos, return_attn=True, temperature=temperature)
        else:
            a = self.attn(self.norm1(x), pos=pos)
        x = x + self.ls1(a)
        x = x + self.ls2(self.mlp(self.norm2(x)))
        return (x, maps) if return_attn else x


class _PatchEmbed(nn.Module):
    def __init__(self, patch, dim):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, kernel_size=patch, stride=patch)

    def forward(self, x):
        return self.proj(x).flatten(2).transpose(1, 2)


class AggregatorLayout(nn.Module):
    """Frame / global alternating attention with a camera token and register tokens per view (the first view's own, the others' shared),
    the layout of the VGGT teacher's aggregator: forward(images [B, S, 3, H, W]) -> (per-depth [frame | global] tokens, prefix, attn_mean)."""

    def __init__(self, img_size, patch_size, embed_dim, depth, num_heads, num_register_tokens, attn_indices, temperature):
        super().__init__()
        self.patch_size, self.attn_indices, self.temperature = patch_size, attn_indices, temperature
        self.patch_start_idx = 1 + num_register_tokens
        self.patch_embed = _PatchEmbed(patch_size, embed_dim)
        self.rope = _Rope2D()
        self.frame_blocks = nn.ModuleList([_Block(embed_dim, num_heads, self.rope) for _ in range(depth)])
        self.global_blocks = nn.ModuleList([_Block(embed_dim, num_heads, self.rope) for _ in range(depth)])
        self.camera_token = nn.Parameter(torch.zeros(1, 2, 1, embed_dim))
        self.register_token = nn.Parameter(torch.zeros(1, 2, num_register_tokens, embed_dim))
        self.register_buffer("mean", torch.tensor([0.485, 0.456, 0.406]).view(1, 1, 3, 1, 1), persistent=False)
        self.register_buffer("std", torch.tensor([0.229, 0.224, 0.225]).view(1, 1, 3, 1, 1), persistent=False)

    @staticmethod
    def _per_view(tok, B, S):
        return torch.cat([tok[:, :1].expand(B, 1, *tok.shape[2:]), tok[:, 1:].expand(B, S - 1, *tok.shape[2:])], dim=1).reshape(B * S, *tok.shape[2:])

    def forward(self, images):
        B, S, _, H, W = images.shape
        x = ((images - self.mean) / self.std).reshape(B * S, 3, H, W)
        tokens = torch.cat([self._per_view(self.camera_token, B, S), self._per_view(self.register_token, B, S), self.patch_embed(x)], dim=1)
        gh, gw = H // self.patch_size, W // self.patch_size
        grid = torch.cartesian_prod(torch.arange(gh), torch.arange(gw)) + 1            # (y, x), the prefix tokens at position 0
        pos = torch.cat([torch.zeros(self.patch_start_idx, 2, dtype=grid.dtype), grid]).expand(B * S, -1, -1)
        _, P, C = tokens.shape
        outputs, maps = [], []
        for i, (fb, gb) in enumerate(zip(self.frame_blocks, self.global_blocks)):
            tokens = fb(tokens.reshape(B * S, P, C), pos=pos)
            frame = tokens.reshape(B, S, P, C)
            tokens, attn = gb(tokens.reshape(B, S * P, C), pos=pos.reshape(B, S * P, 2), return_attn=True, temperature=self.temperature)
            if i in self.attn_indices:
                maps.append(attn)
            outputs.append(torch.cat([frame, tokens.reshape(B, S, P, C)], dim=-1))
        return outputs, self.patch_start_idx, torch.stack(maps).mean(0)


def test_qk_capture_against_reference_aggregator(golden):
    import gd_amd  # noqa: F401
    from gd_amd.teacher_runner import QKCapture, _no_attention_maps
    g = golden("g22_vggt_aggregator")
    agg = AggregatorLayout(**CFG).eval()
    assert ",".join(f"{n}:{'x'.join(map(str, p.shape))}" for n, p in sorted(agg.named_parameters())) == g["param_layout"]
    fill_params(agg)
    img = g["img"]
    with torch.no_grad():
        ref_tokens, ps_idx, ref_attn = agg(img)                       # the reference path: per-head maps materialised
    # the layout reproduces what the reference's own Aggregator returned with the same weights on the same images
    assert ps_idx == 5 and len(ref_tokens) == 3
    for i, t in enumerate(ref_tokens):
        assert float((t - g[f"tokens_{i}"]).abs().max()) < 1e-4 * float(g[f"tokens_{i}"].abs().max()), i
    assert float((ref_attn - g["attn_mean"]).abs().max()) < 1e-6
    sel = [agg.global_blocks[i].attn for i in agg.attn_indices]
    with torch.no_grad(), QKCapture(sel) as cap, _no_attention_maps(sel):
        tokens, ps2, placeholder = agg(img)
    assert ps2 == ps_idx == 5 and placeholder.numel() == 1
    for a, b in zip(tokens, ref_tokens):
        assert torch.equal(a, b)                                      # the teacher's outputs do not change
    qk = cap.pairs()
    assert len(qk) == 2 and qk[0][0].shape == (1, 2, 2 * (5 + 16), 64)
    maps = sum(O.cross_view_attention_maps(q.double(), k.double(), sel[0].scale, 0.8, prefix=5) for q, k in qk) / len(qk)
    want = g["attn_mean"].mean(dim=1)                                 # src/finetune_timm_vggt.py:390-392: head mean of attn.chunk(2)
    assert float((maps - want.double()).abs().max()) < 1e-6
