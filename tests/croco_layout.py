"""A module tree with the layout of the MASt3R teacher's transformer (AsymmetricCroCo3DStereo: CroCo encoder blocks, `decoder_embed`, the two
decoder stacks with cross-attention, `dec_norm`), tiny, test-owned: same attribute and parameter names as the teacher, so `fill_params`
(tests/test_teacher_runner_ref.py) fills it and the reference's own blocks identically, and teacher_blocks.FusedCroCoBlocks reads it as it
reads the user's modules.  Fixture G25 (tools/make_golden_g25.py) pins it against the reference; tests/test_croco_layout_host.py checks that.

Not a test module: imported by test_croco_layout_host.py, test_gpu_mast3r_blocks.py, tools/make_golden_g25.py and tools/bench_teacher.py."""
import torch
import torch.nn as nn
import torch.nn.functional as F

import gd_oracle as O

CFG = dict(enc_dim=192, enc_heads=3, enc_depth=2, dec_dim=128, dec_heads=2, dec_depth=2, temperature=3.0, reciprocity=True)
B, GRID1, GRID2 = 2, (3, 7), (5, 4)          # two views of 21 and 20 tokens
LN_EPS = 1e-6


def grid_positions(batch, gh, gw):
    """int64 [batch, gh * gw, 2] (y, x) of a gh x gw patch grid, row-major."""
    return torch.cartesian_prod(torch.arange(gh), torch.arange(gw)).expand(batch, -1, -1).contiguous()


class DeviceRope2D(nn.Module):
    """2-D RoPE on [B, H, N, D], one instance shared by every block.  On the host it IS gd_oracle.rope_2d; on the GPU the same arithmetic with the
    frequency table on the tokens' device (the oracle builds it on the host)."""

    def __init__(self, base=100.0):
        super().__init__()
        self.base = base

    def forward(self, tokens, positions):
        if not tokens.is_cuda:
            return O.rope_2d(tokens.transpose(1, 2), positions, self.base).transpose(1, 2)
        Q, positions = tokens.shape[-1] // 4, positions.to(tokens.device)
        inv = 1.0 / (self.base ** (torch.arange(Q, dtype=torch.float32, device=tokens.device) / Q))
        out = tokens.clone()
        for ax in range(2):
            th = positions[..., ax].float().unsqueeze(-1) * inv                       # [B, N, Q]
            c, s = torch.cos(th).unsqueeze(1), torch.sin(th).unsqueeze(1)
            u, v = tokens[..., 2 * ax * Q:(2 * ax + 1) * Q], tokens[..., (2 * ax + 1) * Q:(2 * ax + 2) * Q]
            out[..., 2 * ax * Q:(2 * ax + 1) * Q] = u * c - v * s
            out[..., (2 * ax + 1) * Q:(2 * ax + 2) * Q] = v * c + u * s
        return out


def _heads(t, H):
    b, n, c = t.shape
    return t.reshape(b, n, H, c // H).transpose(1, 2)


class _SelfAttention(nn.Module):
    def __init__(self, dim, heads, rope):
        super().__init__()
        self.num_heads, self.scale, self.rope = heads, (dim // heads) ** -0.5, rope
        self.qkv, self.proj = nn.Linear(dim, 3 * dim, bias=True), nn.Linear(dim, dim)

    def forward(self, x, xpos):
        q, k, v = (_heads(t, self.num_heads) for t in self.qkv(x).chunk(3, dim=-1))
        if self.rope is not None:
            q, k = self.rope(q, xpos), self.rope(k, xpos)
        p = F.softmax(q @ k.transpose(-2, -1) * self.scale, dim=-1)
        return self.proj((p @ v).transpose(1, 2).reshape(x.shape))


class _CrossAttention(nn.Module):
    def __init__(self, dim, heads, rope):
        super().__init__()
        self.num_heads, self.scale, self.rope = heads, (dim // heads) ** -0.5, rope
        self.projq, self.projk, self.projv = nn.Linear(dim, dim, bias=True), nn.Linear(dim, dim, bias=True), nn.Linear(dim, dim, bias=True)
        self.proj = nn.Linear(dim, dim)

    def forward(self, query, key, value, qpos, kpos):
        """-> (output [B, Nq, C], the raw scaled scores [B, H, Nq, Nk])"""
        q, k, v = _heads(self.projq(query), self.num_heads), _heads(self.projk(key), self.num_heads), _heads(self.projv(value), self.num_heads)
        if self.rope is not None:
            q, k = self.rope(q, qpos), self.rope(k, kpos)
        scores = q @ k.transpose(-2, -1) * self.scale
        out = (F.softmax(scores, dim=-1) @ v).transpose(1, 2).reshape(query.shape)
        return self.proj(out), scores.detach().clone()


class _Mlp(nn.Module):
    def __init__(self, dim, act=None):
        super().__init__()
        self.fc1, self.act, self.fc2 = nn.Linear(dim, 4 * dim), act or nn.GELU(), nn.Linear(4 * dim, dim)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class CrocoBlock(nn.Module):
    def __init__(self, dim, heads, rope, act=None):
        super().__init__()
        self.norm1, self.norm2 = nn.LayerNorm(dim, eps=LN_EPS), nn.LayerNorm(dim, eps=LN_EPS)
        self.attn, self.mlp = _SelfAttention(dim, heads, rope), _Mlp(dim, act)

    def forward(self, x, xpos):
        x = x + self.attn(self.norm1(x), xpos)
        return x + self.mlp(self.norm2(x))


class CrocoDecoderBlock(nn.Module):
    def __init__(self, dim, heads, rope, norm_mem=True, act=None):
        super().__init__()
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(dim, eps=LN_EPS), nn.LayerNorm(dim, eps=LN_EPS), nn.LayerNorm(dim, eps=LN_EPS)
        self.norm_y = nn.LayerNorm(dim, eps=LN_EPS) if norm_mem else nn.Identity()
        self.attn, self.cross_attn, self.mlp = _SelfAttention(dim, heads, rope), _CrossAttention(dim, heads, rope), _Mlp(dim, act)

    def forward(self, x, y, xpos, ypos):
        """x: this view's tokens, y: the other view's (memory) -> (x, y, raw cross-attention scores [B, H, Nx, Ny])"""
        x = x + self.attn(self.norm1(x), xpos)
        mem = self.norm_y(y)
        a, scores = self.cross_attn(self.norm2(x), mem, mem, xpos, ypos)
        x = x + a
        return x + self.mlp(self.norm3(x)), y, scores


class CrocoLayout(nn.Module):
    def __init__(self, enc_dim, enc_heads, enc_depth, dec_dim, dec_heads, dec_depth, temperature, reciprocity, dec_depth2=None):
        super().__init__()
        self.rope = DeviceRope2D(100.0)
        self.enc_blocks = nn.ModuleList([CrocoBlock(enc_dim, enc_heads, self.rope) for _ in range(enc_depth)])
        self.enc_norm = nn.LayerNorm(enc_dim, eps=LN_EPS)
        self.decoder_embed = nn.Linear(enc_dim, dec_dim, bias=True)
        self.dec_blocks = nn.ModuleList([CrocoDecoderBlock(dec_dim, dec_heads, self.rope) for _ in range(dec_depth)])
        self.dec_blocks2 = nn.ModuleList([CrocoDecoderBlock(dec_dim, dec_heads, self.rope) for _ in range(dec_depth if dec_depth2 is None else dec_depth2)])
        self.dec_norm = nn.LayerNorm(dec_dim, eps=LN_EPS)
        self.temperature, self.reciprocity = temperature, reciprocity

    def encode_blocks(self, x, pos):
        """the encoder blocks alone (what FusedCroCoBlocks.encode replaces); `enc_norm` follows in `encode`"""
        for blk in self.enc_blocks:
            x = blk(x, pos)
        return x

    def encode(self, x, pos):
        return self.enc_norm(self.encode_blocks(x, pos))

    def _decoder(self, f1, pos1, f2, pos2):
        """-> ([view-1 outputs, view-2 outputs], per-layer scores of view 1 on view 2 [B, H, N1, N2], of view 2 on view 1 [B, H, N2, N1]).
        The outputs: the encoder features, then every layer's result, the last one through `dec_norm`.  Both sides of a layer read the
        previous layer's pair."""
        pairs = [(f1, f2)]
        x1, x2 = self.decoder_embed(f1), self.decoder_embed(f2)
        maps1, maps2 = [], []
        for blk1, blk2 in zip(self.dec_blocks, self.dec_blocks2):
            n1, _, s1 = blk1(x1, x2, pos1, pos2)
            n2, _, s2 = blk2(x2, x1, pos2, pos1)
            x1, x2 = n1, n2
            pairs.append((x1, x2))
            maps1.append(s1)
            maps2.append(s2)
        pairs[-1] = (self.dec_norm(x1), self.dec_norm(x2))
        return list(zip(*pairs)), maps1, maps2

    def target_from_maps(self, maps1, maps2):
        """`tgt_attn_map` from the decoder's score maps: head mean, reciprocity average, softmax at `temperature`, column 0 := the layer map's
        minimum, layer mean (gd_oracle.mast3r_tgt_attn_map holds the arithmetic) -> [B, N1, N2]"""
        return O.mast3r_tgt_attn_map(maps1, maps2, self.temperature, self.reciprocity)

    def target(self, f1, pos1, f2, pos2, decoder=None):
        """(decoder outputs, tgt_attn_map) — `decoder`: what stands in for `_decoder` (e.g. one returning head-mean maps)"""
        outs, maps1, maps2 = (decoder or self._decoder)(f1, pos1, f2, pos2)
        return outs, self.target_from_maps(maps1, maps2)


def param_layout(module):
    return ",".join(f"{n}:{'x'.join(map(str, p.shape))}" for n, p in sorted(module.named_parameters()))


def seeded_inputs(seed=250):
    """N(0, 1) tokens after the patch embedding for the two views, and their grid positions: (x1, pos1, x2, pos2)"""
    g = torch.Generator().manual_seed(seed)
    n1, n2 = GRID1[0] * GRID1[1], GRID2[0] * GRID2[1]
    return (torch.randn(B, n1, CFG["enc_dim"], generator=g), grid_positions(B, *GRID1),
            torch.randn(B, n2, CFG["enc_dim"], generator=g), grid_positions(B, *GRID2))
