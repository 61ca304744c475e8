"""A test-owned module tree with the attribute and parameter names of the VGGT teacher's dense-prediction head (vggt/heads/dpt_head.py DPTHead:
`norm`, `projects`, `resize_layers`, `scratch.layer{1..4}_rn`, `scratch.refinenet{1..4}` with `resConfUnit1/2.conv1/2` and `out_conv`,
`scratch.output_conv1/2`), written from the head's published structure (Ranftl et al., "Vision Transformers for Dense Prediction") so that
`fill_params` of tests/test_teacher_runner_ref.py fills it and the reference's own head by name with the same numbers.  Fixture G26
(tools/make_golden_g26.py) holds what the REFERENCE's DPTHead returned; tests/test_dpt_layout_host.py holds this tree to it.

The three fixture cases and their seeded inputs live here, so that the generator and every test build the same tensors."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

PATCH, PREFIX, FRAMES, DIM_IN, FEATURES, OUT_CHANNELS, LAYER_IDX = 14, 5, 2, 32, 16, [16, 32, 64, 64], [0, 1, 2, 3]
CASES = {
    "a": dict(grid=(3, 5), output_dim=2, activation="exp", conf_activation="expp1", feature_only=False, down_ratio=1),
    "b": dict(grid=(4, 4), output_dim=4, activation="inv_log", conf_activation="expp1", feature_only=False, down_ratio=1),
    "c": dict(grid=(3, 5), output_dim=2, activation="exp", conf_activation="expp1", feature_only=True, down_ratio=2),
}


def sincos_table(coords, channels):
    """coords [n] -> [n, channels] float32: [sin | cos] of coord * 100^(-j / (channels / 2)), the angles in fp64."""
    half = channels // 2
    omega = 1.0 / 100.0 ** (torch.arange(half, dtype=torch.float64) / half)
    ang = coords.reshape(-1, 1) * omega            # (a float32 coordinate times fp64 frequencies: the product is fp64)
    return torch.cat([ang.sin(), ang.cos()], dim=1).float()


def pos_tables(gw, gh, channels, aspect, ratio=0.1):
    """The head's position embedding of a gh x gw map is separable: channels [:C/2] depend on x alone, [C/2:] on y alone.
    -> (px [gw, C/2], py [gh, C/2]) float32, `ratio` applied.  The coordinates span +-span * (n - 1) / n with the spans of a unit-diagonal
    rectangle of the IMAGE's aspect ratio, and are float32 numbers (the head builds them in the map's dtype)."""
    diag = (aspect ** 2 + 1.0) ** 0.5
    sx, sy = aspect / diag, 1.0 / diag
    xs = torch.linspace(-sx * (gw - 1) / gw, sx * (gw - 1) / gw, steps=gw, dtype=torch.float32)
    ys = torch.linspace(-sy * (gh - 1) / gh, sy * (gh - 1) / gh, steps=gh, dtype=torch.float32)
    return sincos_table(xs, channels // 2) * ratio, sincos_table(ys, channels // 2) * ratio


def add_pos(x, img_w, img_h):
    """x [N, C, h, w] + the embedding of its own grid at the image's aspect ratio."""
    _, C, h, w = x.shape
    px, py = pos_tables(w, h, C, img_w / img_h)
    emb = torch.cat([px[None].expand(h, w, C // 2), py[:, None].expand(h, w, C // 2)], dim=-1)
    return x + emb.permute(2, 0, 1)[None].to(device=x.device, dtype=x.dtype)


def upsample(x, size=None, scale=None):
    if size is None:
        size = (int(x.shape[-2] * scale), int(x.shape[-1] * scale))
    return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=True)


class ResidualUnit(nn.Module):
    """skip + conv2(relu(conv1(relu(x)))), two 3x3 convolutions.  The teacher builds its units with ReLU(inplace=True), which rectifies the unit's
    input before the skip reads it: skip = relu(x).  With an out-of-place activation the skip is x itself.  (`activation` is only read for its
    `inplace` flag; this forward never writes into its input.)"""

    def __init__(self, features, inplace=True):
        super().__init__()
        self.bn, self.groups, self.norm1, self.norm2 = False, 1, None, None
        self.conv1 = nn.Conv2d(features, features, 3, padding=1)
        self.conv2 = nn.Conv2d(features, features, 3, padding=1)
        self.activation = nn.ReLU(inplace=inplace)

    def forward(self, x):
        r = F.relu(x)
        return (r if self.activation.inplace else x) + self.conv2(F.relu(self.conv1(r)))


class FusionBlock(nn.Module):
    """(previous output [+ resConfUnit1(skip)]) -> resConfUnit2 -> bilinear upsampling (align_corners) -> 1x1 out_conv."""

    def __init__(self, features, has_residual=True, inplace=True):
        super().__init__()
        self.deconv, self.expand, self.align_corners, self.groups, self.size, self.has_residual = False, False, True, 1, None, has_residual
        self.out_conv = nn.Conv2d(features, features, 1)
        if has_residual:
            self.resConfUnit1 = ResidualUnit(features, inplace)
        self.resConfUnit2 = ResidualUnit(features, inplace)

    def forward(self, x, skip=None, size=None):
        if self.has_residual:
            x = x + self.resConfUnit1(skip)
        x = self.resConfUnit2(x)
        return self.out_conv(upsample(x, size=size, scale=None if size is not None else 2))


class DPTLayout(nn.Module):
    def __init__(self, dim_in=DIM_IN, patch_size=PATCH, output_dim=2, activation="exp", conf_activation="expp1", features=FEATURES,
                 out_channels=OUT_CHANNELS, intermediate_layer_idx=LAYER_IDX, pos_embed=True, feature_only=False, down_ratio=1, inplace_relu=True):
        super().__init__()
        self.patch_size, self.activation, self.conf_activation, self.pos_embed = patch_size, activation, conf_activation, pos_embed
        self.feature_only, self.down_ratio, self.intermediate_layer_idx = feature_only, down_ratio, list(intermediate_layer_idx)
        oc = out_channels
        self.norm = nn.LayerNorm(dim_in)
        self.projects = nn.ModuleList([nn.Conv2d(dim_in, c, 1) for c in oc])
        self.resize_layers = nn.ModuleList([nn.ConvTranspose2d(oc[0], oc[0], 4, stride=4), nn.ConvTranspose2d(oc[1], oc[1], 2, stride=2),
                                            nn.Identity(), nn.Conv2d(oc[3], oc[3], 3, stride=2, padding=1)])
        s = nn.Module()
        for i, c in enumerate(oc):
            setattr(s, f"layer{i + 1}_rn", nn.Conv2d(c, features, 3, padding=1, bias=False))
        for i in range(4):
            setattr(s, f"refinenet{i + 1}", FusionBlock(features, has_residual=i != 3, inplace=inplace_relu))
        if feature_only:
            s.output_conv1 = nn.Conv2d(features, features, 3, padding=1)
        else:
            s.output_conv1 = nn.Conv2d(features, features // 2, 3, padding=1)
            s.output_conv2 = nn.Sequential(nn.Conv2d(features // 2, 32, 3, padding=1), nn.ReLU(), nn.Conv2d(32, output_dim, 1))
        self.scratch = s

    def fuse(self, maps):
        s = self.scratch
        rn = [getattr(s, f"layer{i + 1}_rn")(m) for i, m in enumerate(maps)]
        x = s.refinenet4(rn[3], size=rn[2].shape[2:])
        x = s.refinenet3(x, rn[2], size=rn[1].shape[2:])
        x = s.refinenet2(x, rn[1], size=rn[0].shape[2:])
        x = s.refinenet1(x, rn[0])
        return s.output_conv1(x)

    def forward(self, aggregated_tokens_list, images, patch_start_idx, frames_chunk_size=None, taps=None):
        """As the teacher's head: -> (preds [B, S, H, W, output_dim - 1], conf [B, S, H, W]), or features [B, S, C, H', W'] when feature_only.
        Frames are independent, so `frames_chunk_size` changes nothing here.  taps (a dict): receives "pre", the map before the activations
        [B*S, output_dim, H, W] (feature_only: the fused map before the last resampling)."""
        B, S, _, H, W = images.shape
        gh, gw = H // self.patch_size, W // self.patch_size
        maps = []
        for i, li in enumerate(self.intermediate_layer_idx):
            x = self.norm(aggregated_tokens_list[li][:, :, patch_start_idx:].reshape(B * S, gh * gw, -1))
            x = self.projects[i](x.transpose(1, 2).reshape(B * S, -1, gh, gw))
            if self.pos_embed:
                x = add_pos(x, W, H)
            maps.append(self.resize_layers[i](x))
        fused = self.fuse(maps)
        x = upsample(fused, size=(int(gh * self.patch_size / self.down_ratio), int(gw * self.patch_size / self.down_ratio)))
        if self.pos_embed:
            x = add_pos(x, W, H)
        if self.feature_only:
            if taps is not None:
                taps["pre"] = fused
            return x.reshape(B, S, *x.shape[1:])
        y = self.scratch.output_conv2(x)
        if taps is not None:
            taps["pre"] = y
        preds, conf = activate(y.permute(0, 2, 3, 1), self.activation, self.conf_activation)
        return preds.reshape(B, S, *preds.shape[1:]), conf.reshape(B, S, *conf.shape[1:])


def activate(y, activation, conf_activation):
    """y [..., output_dim] -> (values of the first channels, confidence of the last)."""
    v, c = y[..., :-1], y[..., -1]
    v = {"exp": torch.exp, "inv_log": lambda t: torch.sign(t) * torch.expm1(t.abs()), "linear": lambda t: t, "relu": F.relu,
         "sigmoid": torch.sigmoid}[activation](v)
    c = {"expp1": lambda t: 1 + t.exp(), "expp0": torch.exp, "sigmoid": torch.sigmoid}[conf_activation](c)
    return v, c


def make_head(case, **over):
    c = dict(CASES[case])
    c.pop("grid")
    return DPTLayout(**dict(c, **over)).eval()


def seeded_inputs(case):
    """(tokens_list: 4 x [1, FRAMES, PREFIX + gh*gw, DIM_IN], images [1, FRAMES, 3, H, W]) of a fixture case, from a host generator."""
    gh, gw = CASES[case]["grid"]
    g = torch.Generator().manual_seed(2600 + 10 * gh + gw)
    toks = [torch.randn(1, FRAMES, PREFIX + gh * gw, DIM_IN, generator=g) for _ in LAYER_IDX]
    return toks, torch.rand(1, FRAMES, 3, gh * PATCH, gw * PATCH, generator=g)


def param_layout(m):
    return ",".join(f"{n}:{'x'.join(map(str, p.shape))}" for n, p in sorted(m.named_parameters()))


# ----------------------------------------------------------------------------------------------------------------------------------
# A tiny VGGT-shaped teacher around the heads (the runner's tests, CPU and GPU)
# ----------------------------------------------------------------------------------------------------------------------------------
class TinyTrackHead(nn.Module):
    """A track head shaped like the teacher's: `feature_extractor` is a feature-only DPT head (down_ratio 2); the tracker itself is a stub that
    moves every query point one pixel to the right and keeps the feature map it was given (`last_features`).  fail=True: raises after noting
    whether an instance attribute shadows the feature extractor's forward (`saw_shadow`)."""

    def __init__(self, dim_in):
        super().__init__()
        self.feature_extractor = DPTLayout(dim_in=dim_in, feature_only=True, down_ratio=2)
        self.fail, self.saw_shadow, self.last_features = False, None, None

    def forward(self, aggregated_tokens_list, images, patch_start_idx, query_points=None):
        if self.fail:
            self.saw_shadow = "forward" in vars(self.feature_extractor)
            raise RuntimeError("stub track head failure")
        self.last_features = self.feature_extractor(aggregated_tokens_list, images, patch_start_idx)
        q = query_points.float()
        return [torch.stack([q, q + torch.tensor([1.0, 0.0], device=q.device)], dim=1)], None, None


class TinyVGGT(nn.Module):
    """AggregatorLayout (tests/test_teacher_runner_ref.py) + depth / point heads + the track head above + a stub camera head."""
    IMG = (42, 70)          # a 3 x 5 patch grid: aspect ratio != 1

    def __init__(self):
        super().__init__()
        from test_teacher_runner_ref import CFG, AggregatorLayout, fill_params
        self.aggregator = AggregatorLayout(**dict(CFG, depth=4))
        dim = 2 * CFG["embed_dim"]
        self.depth_head = DPTLayout(dim_in=dim, output_dim=2, activation="exp", conf_activation="expp1")
        self.point_head = DPTLayout(dim_in=dim, output_dim=4, activation="inv_log", conf_activation="expp1")
        self.track_head = TinyTrackHead(dim)
        fill_params(self)
        self.eval()

    def camera_head(self, tokens_list):
        return [torch.zeros(1, 2, 9, device=tokens_list[-1].device)]


def tiny_pose_decoder(pose_enc, image_hw):
    """Two identity poses; the second camera's principal point sits half a pixel further, so that no reprojected pixel lands within rounding
    distance of the image border (the co-visibility masks then do not depend on the depth's last bits)."""
    H, W = image_hw
    E = torch.eye(3, 4, device=pose_enc.device).expand(1, 2, 3, 4).contiguous()
    K = torch.tensor([[60.0, 0.0, W / 2], [0.0, 60.0, H / 2], [0.0, 0.0, 1.0]], device=pose_enc.device).expand(1, 2, 3, 3).clone()
    K[0, 1, :2, 2] += 0.5
    return E, K
