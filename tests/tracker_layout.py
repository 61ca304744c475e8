"""A test-owned module tree with the attribute and parameter names of the VGGT teacher's tracker (vggt/heads/track_modules/base_track_predictor.py
BaseTrackerPredictor: `corr_mlp.fc1/fc2`, `query_ref_token`, `updateformer`, `fmap_norm`, `ffeat_norm`, `ffeat_updater`, `vis_predictor`,
`conf_predictor`; its update transformer blocks.py EfficientUpdateFormer: `input_norm`, `input_transform`, `output_norm`, `flow_head`, `virual_tracks`,
`time_blocks`, `space_virtual_blocks`, `space_point2virtual_blocks`, `space_virtual2point_blocks`), written from the tracker's published structure
(Karaev et al., "CoTracker"; Wang et al., "VGGSfM" / "VGGT") so that `fill_params` of tests/test_teacher_runner_ref.py fills it and the reference's own
module by name with the same numbers.  Fixture G28 (tools/make_golden_g28.py) holds what the REFERENCE's tracker returned;
tests/test_tracker_layout_host.py holds this tree to it.

The tree runs in fp32 as the reference does, and in fp64 THROUGHOUT (`.double()`: position table, flow embedding and sampling included), which is what the
GPU tests use as the truth.  `prepare` / `iterate` / `finish` are `forward` cut at the iteration boundary, for the teacher-forced tests.

The fixture cases and their seeded inputs live here, so that the generator and every test build the same tensors."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

LATENT, RADIUS, STRIDE, HIDDEN, DEPTH, ITERS = 128, 4, 2, 96, 2, 4
CASES = {
    "a": dict(B=1, S=2, N=40, H=21, W=35, levels=3),       # small, non-square
    "b": dict(B=1, S=2, N=40, H=131, W=139, levels=7),     # the smallest sides with seven levels; odd sizes drop a row / column at several levels
    "c": dict(B=2, S=3, N=5, H=9, W=11, levels=2),         # frame and batch indexing; query_ref_token on S - 1 frames
}
SEEDS = {"a": 2801, "b": 2802, "c": 2803}


# ----------------------------------------------------------------------------------------------------------------------------------
# sampling and embeddings
# ----------------------------------------------------------------------------------------------------------------------------------
def sample_cells(inp, xy, padding_mode):
    """inp [n, C, H, W], xy [n, h, w, 2] in cell units (x, y) -> [n, C, h, w]: bilinear, align_corners=True.  Cell units become grid_sample's [-1, 1]
    by 2 / max(size - 1, 1) * c - 1."""
    H, W = inp.shape[-2:]
    scale = torch.tensor([2 / max(W - 1, 1), 2 / max(H - 1, 1)], dtype=inp.dtype, device=inp.device)
    return F.grid_sample(inp, xy.to(inp.dtype) * scale - 1, mode="bilinear", padding_mode=padding_mode, align_corners=True)


def sample_points(inp, pts):
    """inp [B, C, H, W], pts [B, R, 2] -> [B, R, C], border padding."""
    return sample_cells(inp, pts[:, :, None, :], "border")[..., 0].transpose(1, 2)


def position_table(dim, H, W, dtype=torch.float32):
    """[1, dim, H, W]: channels [0, dim/2) = [sin | cos](x w_k), [dim/2, dim) the same of y, w_k = 10000^(-k / (dim/4)); computed in fp64 from fp32
    indices, then cast to `dtype` (the reference keeps it in fp32)."""
    q = dim // 4
    omega = 1.0 / 10000 ** (torch.arange(q, dtype=torch.float64) / q)
    ax = torch.arange(W, dtype=torch.float32).double()[:, None] * omega
    ay = torch.arange(H, dtype=torch.float32).double()[:, None] * omega
    ex = torch.cat([ax.sin(), ax.cos()], dim=1)[None].expand(H, W, 2 * q)
    ey = torch.cat([ay.sin(), ay.cos()], dim=1)[:, None].expand(H, W, 2 * q)
    return torch.cat([ex, ey], dim=-1).permute(2, 0, 1)[None].to(dtype)


def flow_embedding(flow, C):
    """flow [M, S, 2] -> [M, S, 2C]: per component, sin / cos interleaved of flow * (2k * 1000 / C), x first."""
    div = (torch.arange(0, C, 2, dtype=torch.float32) * (1000.0 / C)).to(device=flow.device, dtype=flow.dtype)
    out = []
    for comp in (flow[..., 0:1], flow[..., 1:2]):
        a = comp * div
        out.append(torch.stack([a.sin(), a.cos()], dim=-1).flatten(-2))
    return torch.cat(out, dim=-1)


class CorrPyramid:
    """Feature pyramid by repeated 2 x 2 average pooling; `sample` forms each level's full correlation volume and reads the (2r+1)^2 window from it."""

    def __init__(self, fmaps, levels, radius):
        B, S, C, H, W = fmaps.shape
        self.levels, self.radius = levels, radius
        self.maps = [fmaps]
        for _ in range(levels - 1):
            m = self.maps[-1]
            p = F.avg_pool2d(m.flatten(0, 1), 2, stride=2)
            self.maps.append(p.view(B, S, C, *p.shape[-2:]))
        d = torch.linspace(-radius, radius, 2 * radius + 1, device=fmaps.device, dtype=fmaps.dtype)
        # the window offsets: meshgrid "ij" stacked onto an (x, y) centre, so the FIRST window axis moves x
        self.offsets = torch.stack(torch.meshgrid(d, d, indexing="ij"), dim=-1)

    def sample(self, targets, coords):
        """targets [B, S, N, C], coords [B, S, N, 2] (level-0 cells) -> [B, S, N, levels * (2r+1)^2]."""
        B, S, N, C = targets.shape
        out = []
        for l, m in enumerate(self.maps):
            H, W = m.shape[-2:]
            vol = torch.matmul(targets, m.view(B, S, C, H * W)) / math.sqrt(C)
            grid = coords.reshape(B * S * N, 1, 1, 2) / 2 ** l + self.offsets.to(coords.dtype)[None]
            out.append(sample_cells(vol.reshape(B * S * N, 1, H, W), grid, "zeros").view(B, S, N, -1))
        return torch.cat(out, dim=-1)


# ----------------------------------------------------------------------------------------------------------------------------------
# the update transformer
# ----------------------------------------------------------------------------------------------------------------------------------
class _Mlp(nn.Module):
    def __init__(self, dim_in, hidden, dim_out):
        super().__init__()
        self.fc1, self.act, self.fc2 = nn.Linear(dim_in, hidden), nn.GELU(), nn.Linear(hidden, dim_out)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class _SelfBlock(nn.Module):
    """The teacher's block normalises its input IN PLACE of the residual: x = norm1(x); x = x + attn(x); x = x + mlp(norm2(x))."""

    def __init__(self, dim, heads, ratio):
        super().__init__()
        self.norm1, self.norm2 = nn.LayerNorm(dim), nn.LayerNorm(dim)
        self.attn = nn.MultiheadAttention(dim, heads, batch_first=True)
        self.mlp = _Mlp(dim, int(dim * ratio), dim)

    def forward(self, x):
        x = self.norm1(x)
        x = x + self.attn(x, x, x)[0]
        return x + self.mlp(self.norm2(x))


class _CrossBlock(nn.Module):
    def __init__(self, dim, heads, ratio):
        super().__init__()
        self.norm1, self.norm_context, self.norm2 = nn.LayerNorm(dim), nn.LayerNorm(dim), nn.LayerNorm(dim)
        self.cross_attn = nn.MultiheadAttention(dim, heads, batch_first=True)
        self.mlp = _Mlp(dim, int(dim * ratio), dim)

    def forward(self, x, ctx):
        x, ctx = self.norm1(x), self.norm_context(ctx)
        x = x + self.cross_attn(x, ctx, ctx)[0]
        return x + self.mlp(self.norm2(x))


class UpdateFormerLayout(nn.Module):
    """[B, N, T, input_dim] -> ([B, N, T, output_dim], None): attention over time per track, and every few blocks over the tracks of one frame through
    `num_virtual_tracks` learnt virtual tracks (virtual <- points, virtual self, points <- virtual)."""

    def __init__(self, space_depth, time_depth, input_dim, hidden_size, output_dim, num_heads=8, mlp_ratio=4.0, num_virtual_tracks=64):
        super().__init__()
        self.num_virtual_tracks = num_virtual_tracks
        self.input_norm, self.input_transform = nn.LayerNorm(input_dim), nn.Linear(input_dim, hidden_size)
        self.output_norm, self.flow_head = nn.LayerNorm(hidden_size), nn.Linear(hidden_size, output_dim)
        self.virual_tracks = nn.Parameter(torch.randn(1, num_virtual_tracks, 1, hidden_size)) if space_depth else None
        self.time_blocks = nn.ModuleList([_SelfBlock(hidden_size, num_heads, mlp_ratio) for _ in range(time_depth)])
        self.space_virtual_blocks = nn.ModuleList([_SelfBlock(hidden_size, num_heads, mlp_ratio) for _ in range(space_depth)])
        self.space_point2virtual_blocks = nn.ModuleList([_CrossBlock(hidden_size, num_heads, mlp_ratio) for _ in range(space_depth)])
        self.space_virtual2point_blocks = nn.ModuleList([_CrossBlock(hidden_size, num_heads, mlp_ratio) for _ in range(space_depth)])

    def forward(self, x, mask=None):
        tok = self.input_transform(self.input_norm(x))
        first = tok
        B, _, T, D = tok.shape
        nv = self.num_virtual_tracks if self.virual_tracks is not None else 0
        if nv:
            tok = torch.cat([tok, self.virual_tracks.repeat(B, 1, T, 1)], dim=1)
        n = tok.shape[1]
        every = len(self.time_blocks) // max(len(self.space_virtual_blocks), 1)
        j = 0
        for i, blk in enumerate(self.time_blocks):
            tok = blk(tok.reshape(B * n, T, D)).view(B, n, T, D)
            if nv and i % every == 0:
                sp = tok.permute(0, 2, 1, 3).reshape(B * T, n, D)
                pts, virt = sp[:, :n - nv], sp[:, n - nv:]
                virt = self.space_virtual2point_blocks[j](virt, pts)
                virt = self.space_virtual_blocks[j](virt)
                pts = self.space_point2virtual_blocks[j](pts, virt)
                tok = torch.cat([pts, virt], dim=1).view(B, T, n, D).permute(0, 2, 1, 3)
                j += 1
        tok = tok[:, :n - nv] + first
        return self.flow_head(self.output_norm(tok)), None


# ----------------------------------------------------------------------------------------------------------------------------------
# the tracker
# ----------------------------------------------------------------------------------------------------------------------------------
class TrackerLayout(nn.Module):
    """cache_pos_embed: keep the host-built position table on the device after the first call (the reference rebuilds it in every iteration); only the
    bench sets it."""

    def __init__(self, stride=STRIDE, corr_levels=5, corr_radius=RADIUS, latent_dim=LATENT, hidden_size=HIDDEN, use_spaceatt=True, depth=DEPTH, max_scale=518,
                 predict_conf=True, cache_pos_embed=False):
        super().__init__()
        self.stride, self.corr_levels, self.corr_radius, self.latent_dim, self.hidden_size = stride, corr_levels, corr_radius, latent_dim, hidden_size
        self.max_scale, self.predict_conf, self.flows_emb_dim = max_scale, predict_conf, latent_dim // 2
        self.transformer_dim = 3 * latent_dim + 4
        self.cache_pos_embed, self._table = cache_pos_embed, {}
        self.corr_mlp = _Mlp(corr_levels * (2 * corr_radius + 1) ** 2, hidden_size, latent_dim)
        self.query_ref_token = nn.Parameter(torch.randn(1, 2, self.transformer_dim))
        self.updateformer = UpdateFormerLayout(depth if use_spaceatt else 0, depth, self.transformer_dim, hidden_size, latent_dim + 2)
        self.fmap_norm, self.ffeat_norm = nn.LayerNorm(latent_dim), nn.GroupNorm(1, latent_dim)
        self.ffeat_updater = nn.Sequential(nn.Linear(latent_dim, latent_dim), nn.GELU())
        self.vis_predictor = nn.Sequential(nn.Linear(latent_dim, 1))
        if predict_conf:
            self.conf_predictor = nn.Sequential(nn.Linear(latent_dim, 1))

    def _pos_table(self, H, W, ref):
        key = (H, W, ref.dtype, str(ref.device))
        if self.cache_pos_embed and key in self._table:
            return self._table[key]
        t = position_table(self.transformer_dim, H, W, torch.float64 if ref.dtype == torch.float64 else torch.float32).to(ref.device)
        if self.cache_pos_embed:
            self._table[key] = t
        return t

    def prepare(self, query_points, fmaps, down_ratio=1):
        B, S, C, H, W = fmaps.shape
        fmaps = self.fmap_norm(fmaps.permute(0, 1, 3, 4, 2)).permute(0, 1, 4, 2, 3)
        q = query_points / float(down_ratio) if down_ratio > 1 else query_points
        q = q / float(self.stride)
        coords = q[:, None].repeat(1, S, 1, 1)
        qfeat = sample_points(fmaps[:, 0], q)
        return dict(B=B, S=S, N=q.shape[1], H=H, W=W, coords=coords, feats=qfeat[:, None].repeat(1, S, 1, 1), query_feat=qfeat, query=q,
                    pyramid=CorrPyramid(fmaps, self.corr_levels, self.corr_radius), mul=self.stride * (down_ratio if down_ratio > 1 else 1))

    def iterate(self, st):
        """One refinement: st["coords"] / st["feats"] ([B, S, N, .]) are replaced, st["corr"] receives the window samples -> coords at image scale."""
        B, S, N, C = st["B"], st["S"], st["N"], self.latent_dim
        coords, feats = st["coords"], st["feats"]
        st["corr"] = corr = st["pyramid"].sample(feats, coords)
        corr_rows = self.corr_mlp(corr.permute(0, 2, 1, 3).reshape(B * N, S, -1))
        flow = (coords - coords[:, :1]).permute(0, 2, 1, 3).reshape(B * N, S, 2)
        emb = torch.cat([flow_embedding(flow, self.flows_emb_dim), flow / self.max_scale, flow / self.max_scale], dim=-1)
        feat_rows = feats.permute(0, 2, 1, 3).reshape(B * N, S, C)
        x = torch.cat([emb, corr_rows, feat_rows], dim=2)
        table = self._pos_table(st["H"], st["W"], x)
        x = x + sample_points(table.expand(B, -1, -1, -1), st["query"]).reshape(B * N, 1, -1).to(x.dtype)
        tok = self.query_ref_token
        x = x + torch.cat([tok[:, :1], tok[:, 1:2].expand(-1, S - 1, -1)], dim=1).to(x.dtype)
        delta = self.updateformer(x.view(B, N, S, -1))[0].reshape(B * N * S, -1)
        new_feats = self.ffeat_updater(self.ffeat_norm(delta[:, 2:])) + feat_rows.reshape(B * N * S, C)
        st["feats"] = new_feats.view(B, N, S, C).permute(0, 2, 1, 3)
        coords = coords + delta[:, :2].view(B, N, S, 2).permute(0, 2, 1, 3)
        coords[:, 0] = st["query"]
        st["coords"] = coords
        return coords * st["mul"]

    def finish(self, st, apply_sigmoid=True):
        B, S, N = st["B"], st["S"], st["N"]
        rows = st["feats"].reshape(B * S * N, self.latent_dim)
        vis = self.vis_predictor(rows).view(B, S, N)
        conf = self.conf_predictor(rows).view(B, S, N) if self.predict_conf else None
        if apply_sigmoid:
            vis, conf = torch.sigmoid(vis), (torch.sigmoid(conf) if conf is not None else None)
        return vis, conf

    def forward(self, query_points, fmaps=None, iters=6, return_feat=False, down_ratio=1, apply_sigmoid=True, taps=None):
        """As the teacher's tracker.  taps (a dict): receives "corr", the window samples of the first iteration."""
        st = self.prepare(query_points, fmaps, down_ratio)
        preds = []
        for i in range(iters):
            preds.append(self.iterate(st))
            if taps is not None and i == 0:
                taps["corr"] = st["corr"]
        vis, conf = self.finish(st, apply_sigmoid)
        if return_feat:
            return preds, vis, st["feats"], st["query_feat"], conf
        return preds, vis, conf


def condition_weights(tracker):
    """The two coordinate rows of `updateformer.flow_head` times 0.05.  With N(0, 1 / fan-in) rows the loop is chaotic (fp32 against fp64 reaches a pixel
    after four iterations, with the reference's own modules) and no bound means anything; scaled, fp32 stays within 4e-3 px of fp64."""
    with torch.no_grad():
        tracker.updateformer.flow_head.weight[:2] *= 0.05
        tracker.updateformer.flow_head.bias[:2] *= 0.05


def make_tracker(case, seed=28, **over):
    from test_teacher_runner_ref import fill_params
    t = TrackerLayout(**dict(dict(corr_levels=CASES[case]["levels"]), **over))
    fill_params(t, seed=seed)
    condition_weights(t)
    return t.eval()


def seeded_inputs(case):
    """(query_points [B, N, 2] at image scale, fmaps [B, S, LATENT, H, W]) of a fixture case, from a host generator.  Query points are uniform over
    [-3, W + 3] x [-3, H + 3] map cells; the first ones are planted: (0, 0), (W - 1, H - 1), an integer pair, a half-integer pair, one more than
    the radius outside the map."""
    c = CASES[case]
    B, S, N, H, W = c["B"], c["S"], c["N"], c["H"], c["W"]
    g = torch.Generator().manual_seed(SEEDS[case])
    fmaps = torch.randn(B, S, LATENT, H, W, generator=g)
    u = torch.rand(B, N, 2, generator=g)
    q = u * torch.tensor([W + 6.0, H + 6.0]) - 3.0
    planted = torch.tensor([[0.0, 0.0], [W - 1.0, H - 1.0], [3.0, 5.0], [4.5, 2.5], [-(RADIUS + 2.25), 3.25]])
    q[:, :len(planted)] = planted[:N]
    return q * STRIDE, fmaps


def param_layout(m):
    return ",".join(f"{n}:{'x'.join(map(str, p.shape))}" for n, p in sorted(m.named_parameters()))


# ----------------------------------------------------------------------------------------------------------------------------------
# A tiny VGGT-shaped teacher whose track head carries a TrackerLayout (the runner's tests)
# ----------------------------------------------------------------------------------------------------------------------------------
class TrackHeadLayout(nn.Module):
    """`feature_extractor` (a feature-only DPT head at half resolution with LATENT channels) -> `tracker`, `iters` refinements."""

    def __init__(self, dim_in, levels=3, iters=ITERS):
        super().__init__()
        from dpt_layout import DPTLayout
        self.feature_extractor = DPTLayout(dim_in=dim_in, features=LATENT, feature_only=True, down_ratio=2)
        self.tracker = TrackerLayout(stride=2, corr_levels=levels)
        self.iters = iters

    def forward(self, aggregated_tokens_list, images, patch_start_idx, query_points=None, iters=None):
        fm = self.feature_extractor(aggregated_tokens_list, images, patch_start_idx)
        return self.tracker(query_points=query_points, fmaps=fm, iters=self.iters if iters is None else iters)


def make_tiny_vggt(seed=22):
    """dpt_layout.TinyVGGT (42 x 70 images: a 21 x 35 feature map, three pyramid levels) with the track head above."""
    from dpt_layout import TinyVGGT
    from test_teacher_runner_ref import CFG, fill_params

    class TinyVGGTWithTracker(TinyVGGT):
        def __init__(self):
            super().__init__()
            self.track_head = TrackHeadLayout(2 * CFG["embed_dim"])
            fill_params(self, seed=seed)
            condition_weights(self.track_head.tracker)
            self.eval()
    return TinyVGGTWithTracker()
