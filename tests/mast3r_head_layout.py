"""A test-owned module tree with the attribute and parameter names of the MASt3R teacher's head (mast3r/catmlp_dpt_head.py
Cat_MLP_LocalFeatures_DPT_Pts3d: `dpt.act_postprocess[i]`, `dpt.scratch.layer{1..4}_rn`, `dpt.scratch.refinenet{1..4}` with `resConfUnit1/2.conv1/2`
and `out_conv`, `dpt.head`, `head_local_features.fc1/fc2`, and the postprocess attributes `depth_mode`, `conf_mode`, `desc_mode`, `two_confs`,
`desc_conf_mode`, `local_feat_dim`, `patch_size`), written from the head's published structure so that `fill_params` of
tests/test_teacher_runner_ref.py fills it and the reference's own head by name with the same numbers, and teacher_heads.FusedMASt3RHead reads it as it
reads the user's module.  Fixture G27 (tools/make_golden_g27.py) holds what the REFERENCE's head returned; tests/test_mast3r_head_layout_host.py holds
this tree to it.

The fixture cases and their seeded inputs live here, so that the generator and every test build the same tensors.  One frame per case: the frames of a
batch are independent.  The descriptor width differs per case (the three image-size maps of 24 channels each would not fit a committed file): 24
channels on the smallest grid, fewer on the larger ones."""
import torch
import torch.nn as nn
import torch.nn.functional as F

INF = float("inf")
PATCH, ENC, DEC, DEC_DEPTH, FEATURES, LAST_DIM, LAYER_DIMS = 16, 64, 48, 12, 32, 16, (96, 192, 384, 768)
HOOKS = [0, DEC_DEPTH * 2 // 4, DEC_DEPTH * 3 // 4, DEC_DEPTH]
CASES = {
    # both sides odd: refinenet4's doubled output is cropped; the teacher's own modes
    "a": dict(grid=(3, 5), has_conf=True, two_confs=True, local_feat_dim=4, depth_mode=("exp", -INF, INF), conf_mode=("exp", 1, INF),
              desc_conf_mode=("exp", 0, INF)),
    # even; one confidence for both
    "b": dict(grid=(2, 4), has_conf=True, two_confs=False, local_feat_dim=16, depth_mode=("square", -INF, INF), conf_mode=("sigmoid", 0, 5),
              desc_conf_mode=None),
    # one token row, a 1 x 1 stride-2 level; no confidence channel in the adapter, a bounded exp for the descriptors'
    "c": dict(grid=(1, 2), has_conf=False, two_confs=True, local_feat_dim=24, depth_mode=("linear", -INF, INF), conf_mode=None,
              desc_conf_mode=("exp", 0, 20)),
}


class ResidualUnit(nn.Module):
    """x + conv2(relu(conv1(relu(x)))): the activation is out of place, the skip reads x itself."""

    def __init__(self, features):
        super().__init__()
        self.bn, self.groups = False, 1
        self.conv1 = nn.Conv2d(features, features, 3, padding=1)
        self.conv2 = nn.Conv2d(features, features, 3, padding=1)
        self.activation = nn.ReLU(False)

    def forward(self, x):
        return x + self.conv2(self.activation(self.conv1(self.activation(x))))


class FusionBlock(nn.Module):
    """(previous output [+ resConfUnit1(skip)]) -> resConfUnit2 -> bilinear x2 (align_corners) -> 1x1 out_conv.  Every block owns a resConfUnit1;
    the one that gets no skip never runs it."""

    def __init__(self, features):
        super().__init__()
        self.deconv, self.expand, self.align_corners, self.groups, self.width_ratio = False, False, True, 1, 1
        self.out_conv = nn.Conv2d(features, features, 1)
        self.resConfUnit1, self.resConfUnit2 = ResidualUnit(features), ResidualUnit(features)

    def forward(self, x, skip=None):
        if skip is not None:
            x = x + self.resConfUnit1(skip)
        x = F.interpolate(self.resConfUnit2(x), scale_factor=2, mode="bilinear", align_corners=True)
        return self.out_conv(x)


class Interpolate(nn.Module):
    def __init__(self, scale_factor, mode, align_corners):
        super().__init__()
        self.scale_factor, self.mode, self.align_corners = scale_factor, mode, align_corners

    def forward(self, x):
        return F.interpolate(x, scale_factor=self.scale_factor, mode=self.mode, align_corners=self.align_corners)


class Adapter(nn.Module):
    """Four token levels -> 1/4, 1/8, 1/16 and 1/32 of the image (transposed convolutions of stride 4 and 2, nothing, a stride-2 convolution)
    -> `layer_rn` -> refinenet4 .. refinenet1 -> `head`."""

    def __init__(self, num_channels, dim_tokens, hooks, layer_dims=LAYER_DIMS, feature_dim=FEATURES, last_dim=LAST_DIM, patch_size=PATCH):
        super().__init__()
        self.hooks, self.head_type, self.stride_level, self.P_H, self.P_W = list(hooks), "regression", 1, patch_size, patch_size
        d, t = list(layer_dims), list(dim_tokens)
        s = nn.Module()
        for i in range(4):
            setattr(s, f"layer{i + 1}_rn", nn.Conv2d(d[i], feature_dim, 3, padding=1, bias=False))
        s.layer_rn = nn.ModuleList([getattr(s, f"layer{i + 1}_rn") for i in range(4)])
        for i in range(4):
            setattr(s, f"refinenet{i + 1}", FusionBlock(feature_dim))
        self.scratch = s
        self.head = nn.Sequential(nn.Conv2d(feature_dim, feature_dim // 2, 3, padding=1), Interpolate(2, "bilinear", True),
                                  nn.Conv2d(feature_dim // 2, last_dim, 3, padding=1), nn.ReLU(True), nn.Conv2d(last_dim, num_channels, 1))
        self.act_postprocess = nn.ModuleList([
            nn.Sequential(nn.Conv2d(t[0], d[0], 1), nn.ConvTranspose2d(d[0], d[0], 4, stride=4)),
            nn.Sequential(nn.Conv2d(t[1], d[1], 1), nn.ConvTranspose2d(d[1], d[1], 2, stride=2)),
            nn.Sequential(nn.Conv2d(t[2], d[2], 1)),
            nn.Sequential(nn.Conv2d(t[3], d[3], 1), nn.Conv2d(d[3], d[3], 3, stride=2, padding=1))])

    def forward(self, tokens, image_size):
        gh, gw = image_size[0] // (self.stride_level * self.P_H), image_size[1] // (self.stride_level * self.P_W)
        maps = []
        for i, hook in enumerate(self.hooks):
            x = tokens[hook]
            x = x.transpose(1, 2).reshape(x.shape[0], -1, gh, gw)
            maps.append(self.scratch.layer_rn[i](self.act_postprocess[i](x)))
        s = self.scratch
        x = s.refinenet4(maps[3])[:, :, :maps[2].shape[2], :maps[2].shape[3]]          # twice the stride-2 level, cropped to the token grid
        x = s.refinenet3(x, maps[2])
        x = s.refinenet2(x, maps[1])
        return self.head(s.refinenet1(x, maps[0]))


class Mlp(nn.Module):
    def __init__(self, dim, hidden, out):
        super().__init__()
        self.fc1, self.act, self.fc2 = nn.Linear(dim, hidden), nn.GELU(), nn.Linear(hidden, out)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


def points(xyz, mode):
    """xyz [..., 3] -> pts3d.  'linear': itself; else direction * f(length), f = square | expm1; the length is clipped at 1e-8 in the division only."""
    kind, vmin, vmax = mode
    assert vmin == -INF and vmax == INF
    if kind == "linear":
        return xyz
    d = xyz.norm(dim=-1, keepdim=True)
    u = xyz / d.clip(min=1e-8)
    return u * (d.square() if kind == "square" else torch.expm1(d))


def confidence(y, mode):
    kind, vmin, vmax = mode
    if kind == "exp":
        return vmin + y.exp().clip(max=vmax - vmin)
    assert kind == "sigmoid"
    return (vmax - vmin) * torch.sigmoid(y) + vmin


def postprocess(out, depth_mode, conf_mode, desc_dim=None, desc_mode="norm", two_confs=False, desc_conf_mode=None):
    """out [B, 3 + has_conf + D + two_confs, H, W] -> the head's dict.  The descriptor is divided by its norm with no epsilon."""
    assert "norm" in desc_mode
    fmap = out.permute(0, 2, 3, 1)
    res = dict(pts3d=points(fmap[..., 0:3], depth_mode))
    if conf_mode is not None:
        res["conf"] = confidence(fmap[..., 3], conf_mode)
    start = 3 + int(conf_mode is not None)
    d = fmap[..., start:start + desc_dim]
    res["desc"] = d / d.norm(dim=-1, keepdim=True)
    res["desc_conf"] = confidence(fmap[..., start + desc_dim], conf_mode if desc_conf_mode is None else desc_conf_mode) if two_confs else res["conf"].clone()
    return res


class MASt3RHeadLayout(nn.Module):
    def __init__(self, has_conf=True, two_confs=True, local_feat_dim=24, depth_mode=("exp", -INF, INF), conf_mode=("exp", 1, INF),
                 desc_conf_mode=("exp", 0, INF), desc_mode="norm", enc_dim=ENC, dec_dim=DEC, hooks=HOOKS, feature_dim=FEATURES, last_dim=LAST_DIM,
                 layer_dims=LAYER_DIMS, patch_size=PATCH, hidden_dim_factor=4.0):
        super().__init__()
        self.postprocess, self.depth_mode, self.conf_mode, self.desc_mode, self.desc_conf_mode = postprocess, depth_mode, conf_mode, desc_mode, desc_conf_mode
        self.has_conf, self.two_confs, self.local_feat_dim, self.patch_size = has_conf, two_confs, local_feat_dim, patch_size
        self.dpt = Adapter(3 + has_conf, [enc_dim, dec_dim, dec_dim, dec_dim], hooks, layer_dims, feature_dim, last_dim, patch_size)
        idim = enc_dim + dec_dim
        self.head_local_features = Mlp(idim, int(hidden_dim_factor * idim), (local_feat_dim + two_confs) * patch_size ** 2)

    def forward(self, decout, img_shape, taps=None):
        """decout: the list of [B, gh*gw, C] outputs (encoder first, then every decoder layer); img_shape (H, W).
        taps (a dict): receives "pre", the map before the postprocess [B, 3 + has_conf + D + two_confs, H, W]."""
        H, W = img_shape
        pts = self.dpt(decout, image_size=(H, W))
        cat = torch.cat([decout[0], decout[-1]], dim=-1)
        lf = self.head_local_features(cat).transpose(-1, -2).reshape(cat.shape[0], -1, H // self.patch_size, W // self.patch_size)
        out = torch.cat([pts, F.pixel_shuffle(lf, self.patch_size)], dim=1)
        if taps is not None:
            taps["pre"] = out
        if self.postprocess:
            out = self.postprocess(out, depth_mode=self.depth_mode, conf_mode=self.conf_mode, desc_dim=self.local_feat_dim, desc_mode=self.desc_mode,
                                   two_confs=self.two_confs, desc_conf_mode=self.desc_conf_mode)
        return out


def make_head(case, **over):
    c = dict(CASES[case])
    c.pop("grid")
    return MASt3RHeadLayout(**dict(c, **over)).eval()


def seeded_inputs(case):
    """(decout: DEC_DEPTH + 1 tensors [1, gh*gw, ENC | DEC], (H, W)) of a fixture case, from a host generator."""
    gh, gw = CASES[case]["grid"]
    g = torch.Generator().manual_seed(2700 + 10 * gh + gw)
    return [torch.randn(1, gh * gw, ENC if i == 0 else DEC, generator=g) for i in range(DEC_DEPTH + 1)], (gh * PATCH, gw * PATCH)


def param_layout(m):
    return ",".join(f"{n}:{'x'.join(map(str, p.shape))}" for n, p in sorted(m.named_parameters()))


# ----------------------------------------------------------------------------------------------------------------------------------
# A tiny MASt3R-shaped matcher around two heads (the runner's tests, CPU and GPU)
# ----------------------------------------------------------------------------------------------------------------------------------
IMG_H, IMG_W = 48, 80          # a 3 x 5 patch grid


def tiny_matcher(cfg=None, img_hw=(IMG_H, IMG_W), head_kw=None, fill=True):
    """CrocoLayout (tests/croco_layout.py) with four decoder layers + a linear patch embedding + `downstream_head1/2` (the layout above, D = 24, the
    teacher's modes) + `head1` / `head2` closures that call those modules, as the teacher's portrait / landscape wrappers do.  The two decoder stacks
    and the two heads carry the same weights, so a pair of equal images gets equal descriptors in both views: every pixel's reciprocal nearest
    neighbour is its twin, by a margin that no rounding closes.  `fail`: forward raises after noting which heads carry an instance `forward`
    (`saw_shadow`).  cfg / img_hw / head_kw: another size (tools/bench_teacher.py); fill=False keeps torch's own initialisation."""
    import croco_layout as CL
    from test_teacher_runner_ref import fill_params
    cfg = dict(CL.CFG, dec_depth=4) if cfg is None else cfg
    L = cfg["dec_depth"]
    kw = dict(dict(enc_dim=cfg["enc_dim"], dec_dim=cfg["dec_dim"], hooks=[0, L * 2 // 4, L * 3 // 4, L], layer_dims=(16, 24, 32, 32)), **(head_kw or {}))
    H, W = img_hw

    class TinyMatcher(CL.CrocoLayout):
        def __init__(self):
            super().__init__(**cfg)
            self.patch_embed = nn.Linear(3 * PATCH * PATCH, cfg["enc_dim"])
            self.downstream_head1, self.downstream_head2 = MASt3RHeadLayout(**kw), MASt3RHeadLayout(**kw)
            self.head1 = lambda decout, shape: self.downstream_head1(decout, shape)
            self.head2 = lambda decout, shape: self.downstream_head2(decout, shape)
            self.fail, self.saw_shadow = False, None

        def _encode_image(self, img):
            b, gh, gw = img.shape[0], H // PATCH, W // PATCH
            x = self.patch_embed(img.reshape(b, 3, gh, PATCH, gw, PATCH).permute(0, 2, 4, 1, 3, 5).reshape(b, gh * gw, -1))
            pos = CL.grid_positions(b, gh, gw).to(img.device)
            for blk in self.enc_blocks:
                x = blk(x, pos)
            return self.enc_norm(x), pos

        def forward(self, view1, view2):
            (f1, pos1), (f2, pos2) = self._encode_image(view1["img"]), self._encode_image(view2["img"])
            dec, maps1, maps2 = self._decoder(f1, pos1, f2, pos2)
            if self.fail:
                self.saw_shadow = ["forward" in vars(self.downstream_head1), "forward" in vars(self.downstream_head2)]
                raise RuntimeError("stub matcher failure")
            res1 = self.head1([t.float() for t in dec[0]], (H, W))          # the teacher runs its heads in fp32, autocast off
            res2 = self.head2([t.float() for t in dec[1]], (H, W))
            res2["pts3d_in_other_view"] = res2.pop("pts3d")
            res2["tgt_attn_map"] = self.target_from_maps(maps1, maps2)
            return res1, res2

    m = TinyMatcher().eval()
    if fill:
        fill_params(m, seed=27)
    m.dec_blocks2.load_state_dict(m.dec_blocks.state_dict())
    m.downstream_head2.load_state_dict(m.downstream_head1.state_dict())
    return m


def make_pairs(imgs, scene_graph="complete", prefilter=None, symmetrize=True):
    return [(imgs[0], imgs[1]), (imgs[1], imgs[0])]


def inference(pairs, model, device, verbose=False):
    v1 = {"img": torch.cat([a for a, _ in pairs]).to(device)}
    v2 = {"img": torch.cat([b for _, b in pairs]).to(device)}
    p1, p2 = model(v1, v2)
    return {"view1": v1, "view2": v2, "pred1": p1, "pred2": p2}
