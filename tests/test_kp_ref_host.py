"""tests/kp_ref64.py checked on the CPU: the fp64 restatements against the oracle (F.grid_sample, gd_oracle, autograd of both), the exactness of the
dyadic geometry in fp32 arithmetic, and that the bounds are tight enough AT THE GPU TESTS' OWN INPUTS for a list of wrong references to fail them."""
import gd_oracle as O
import pytest
import torch
import torch.nn.functional as F

import kp_ref64 as K
from rowwise_ref64 import conv_weight_pack_ref

F64 = torch.float64
# stride != patch, image no multiple of either: gh = (75 - 14) // 7 + 1, gw = (101 - 14) // 7 + 1
STRIDED = dict(gh=9, gw=13, patch=14, stride=7, img_h=75, img_w=101, sx=K._f32(0.9), sy=K._f32(1.7))
ORACLE_GEOMS = [K.GEOMS["generic"], K.GEOMS["exact"], K.GEOMS["tiny"], STRIDED]


def _kp(geom, Nk=40, seed=3):
    """Inside, on the border, outside, -1-padded (probe_keypoints has them all)."""
    return K.probe_keypoints(geom, 2, Nk, seed)


def _W(kp, geom):
    c = K.gather_consts(geom["img_h"], geom["img_w"], geom["patch"], geom["stride"])
    gx, gy = K.coords64(kp, geom["sx"], geom["sy"], c, geom["gh"], geom["gw"])
    return K.weights64(gx, gy, geom["gh"], geom["gw"]), gx, gy


def _model_px(kp, geom):
    return kp.double() * torch.tensor([geom["sx"], geom["sy"]], dtype=F64)


def _oracle_sample(fmap, kp, geom):
    """gd_oracle.interpolate_features on a [B, gh, gw, D] fp64 map -> [B, Nk, D]."""
    out = O.interpolate_features(fmap.permute(0, 3, 1, 2), _model_px(kp, geom).float(), geom["img_h"], geom["img_w"], normalize=False,
                                 patch_size=geom["patch"], stride=geom["stride"])
    return out.transpose(1, 2)


def _grid_sample(fmap, kp, geom):
    ax, bx, ay, by = K.gather_consts(geom["img_h"], geom["img_w"], geom["patch"], geom["stride"])
    p = _model_px(kp, geom)
    g = torch.stack([ax * p[..., 0] + bx, ay * p[..., 1] + by], -1)[:, None]              # [B, 1, Nk, 2]
    out = F.grid_sample(fmap.permute(0, 3, 1, 2), g, mode="bilinear", padding_mode="border", align_corners=True)
    return out[:, :, 0].transpose(1, 2)


@pytest.mark.parametrize("gi", range(len(ORACLE_GEOMS)))
def test_gather_is_grid_sample_and_the_oracle(gi):
    geom = ORACLE_GEOMS[gi]
    kp = _kp(geom)
    W, _, _ = _W(kp, geom)
    assert torch.allclose(W.sum((-1, -2)), torch.ones(2, 40, dtype=F64), atol=1e-14), "the weights of a keypoint sum to 1"
    grids = [K.cover_grid(geom, 2, 5, 50 + t).double() for t in range(3)]
    ref = K.gather_fwd64(grids, W)
    gs = sum(_grid_sample(g, kp, geom) for g in grids) / 3
    assert (ref - gs).abs().max() < 1e-12
    # the oracle forms a * pts.float() + b in fp32 (the first three roundings of gather_coords) and the rest in fp64: inside the coordinate bound
    orc = sum(_oracle_sample(g, kp, geom) for g in grids) / 3
    _, dW = K.geometry64(kp, geom)
    assert ((ref - orc).abs() <= K.gather_fwd_bound(grids, W, dW)).all()


@pytest.mark.parametrize("gi", range(len(ORACLE_GEOMS)))
def test_scatter_is_autograd_of_grid_sample(gi):
    geom = ORACLE_GEOMS[gi]
    kp = _kp(geom)
    W, _, _ = _W(kp, geom)
    fmap = K.cover_grid(geom, 2, 5, 60).double().requires_grad_(True)
    dout = torch.randn(2, 40, 5, dtype=F64, generator=torch.Generator().manual_seed(61))
    (_grid_sample(fmap, kp, geom) * dout).sum().backward()
    for prefix, extra in ((0, 0), (1, 1)):
        pitch = geom["gw"] + extra
        got = K.gather_bwd64(dout, W, 0.25, prefix, pitch)
        assert got.shape == (2, prefix + geom["gh"] * pitch, 5)
        assert (got - K.embed(fmap.grad * 0.25, prefix, pitch)).abs().max() < 1e-12
        assert got[:, :prefix].abs().max() == 0 if prefix else True
        assert got[:, prefix:].view(2, geom["gh"], pitch, 5)[:, :, geom["gw"]:].abs().sum() == 0


@pytest.mark.parametrize("gi", range(len(ORACLE_GEOMS)))
def test_patch_gather_is_conv_then_sample_and_its_transpose(gi):
    geom = ORACLE_GEOMS[gi]
    kp = _kp(geom)
    W, _, _ = _W(kp, geom)
    D = 4
    g = torch.Generator().manual_seed(70)
    fmap = K.cover_grid(geom, 2, D, 71).double().requires_grad_(True)
    w = torch.randn(D, D, 3, 3, dtype=F64, generator=g)
    wk = conv_weight_pack_ref(w, F64)[0]                                          # [n, (ky, kx, c)]
    conv = F.conv2d(fmap.permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1)
    ref = _grid_sample(conv, kp, geom)                                            # [B, Nk, n]
    got = K.patch_gather64(fmap.detach(), W) @ wk.t()
    assert (got.view(2, 40, D) - ref).abs().max() < 1e-11
    dfeat = torch.randn(2, 40, D, dtype=F64, generator=g)
    (ref * dfeat).sum().backward()
    U9 = dfeat.view(80, D) @ wk                                                   # [B Nk, 9 D]
    back = K.patch_bwd64(U9, W, prefix=1)
    assert back[:, 0].abs().max() == 0
    assert (back[:, 1:].view(2, geom["gh"], geom["gw"], D) - fmap.grad).abs().max() < 1e-11
    # and as a bilinear form: <patch_gather(x), U> == <x, patch_bwd(U)>
    lhs = (K.patch_gather64(fmap.detach(), W) * U9).sum()
    rhs = (fmap.detach() * K.patch_bwd64(U9, W).view(2, geom["gh"], geom["gw"], D)).sum()
    assert abs(lhs - rhs) < 1e-10 * abs(lhs)


def test_ln_gather_is_gather_of_layernorm():
    geom = K.GEOMS["generic"]
    kp = _kp(geom)
    W, _, _ = _W(kp, geom)
    grids = [K.cover_grid(geom, 2, 16, 80 + t) * 3 + 40 for t in range(2)]
    gm, bt = torch.randn(16), torch.randn(16)
    st = [(g.double().mean(-1).float(), (g.double().var(-1, unbiased=False) + 1e-6).rsqrt().float()) for g in grids]
    got = K.gather_ln_fwd64(grids, [s[0] for s in st], [s[1] for s in st], gm, bt, W)
    ref = K.gather_fwd64([F.layer_norm(g.double(), (16,), gm.double(), bt.double(), 1e-6) for g in grids], W)
    assert (got - ref).abs().max() < 1e-5                                         # the statistics handed over are fp32
    assert (K.gather_ln_fwd_bound(grids, [s[0] for s in st], [s[1] for s in st], gm, bt, W, torch.zeros_like(W)) > 0).all()


def test_kp_depth_is_the_oracle_for_in_image_keypoints():
    g = torch.Generator().manual_seed(90)
    H, Wd = 7, 10
    depth = torch.rand(2, H, Wd, generator=g) * 5
    kp = torch.stack([torch.randint(0, Wd, (2, 30), generator=g), torch.randint(0, H, (2, 30), generator=g)], -1).float()
    kp[0, 0], kp[0, 1] = torch.tensor([0.0, 0.0]), torch.tensor([Wd - 1.0, H - 1.0])
    got = K.kp_depth64(depth, kp)
    for b in range(2):
        ref = O.extract_kp_depth(depth[b].double(), kp[b:b + 1])
        assert (got[b] - ref[0]).abs().max() < 1e-13
    # padded and out-of-image keypoints clamp into the image: -1 -> (0, 0), beyond -> the last pixel
    out = K.kp_depth64(depth, torch.tensor([[[-1.0, -1.0], [50.0, 50.0]]]).expand(2, 2, 2))
    assert torch.equal(out[:, 0], K.kp_depth64(depth, torch.zeros(2, 1, 2))[:, 0])
    assert torch.equal(out[:, 1], K.kp_depth64(depth, torch.tensor([[[Wd - 1.0, H - 1.0]]]).expand(2, 1, 2))[:, 0])
    assert (K.kp_depth_bound(depth, kp) > 0).all()


def test_patch_mask_ref_is_the_oracle_where_every_keypoint_has_a_patch():
    g = torch.Generator().manual_seed(91)
    H, Wd, P = 56, 70, 14
    kp = torch.rand(2, 25, 2, generator=g) * torch.tensor([Wd + 20.0, H + 20.0]) - 10
    kp[1, 20:] = -1.0
    got = K.patch_mask_ref(kp, H, Wd, P)
    for b in range(2):
        assert torch.equal(got[b].bool(), O.patch_mask_from_kp(kp[b], H, Wd, P))
    # the remainder strip (H, W no multiples of P) marks nothing; x = W - 0.5 is inside the image, x = W and x = -0.5 are not
    kp = torch.tensor([[[59.5, 3.0], [60.0, 3.0], [-0.5, 3.0], [57.0, 3.0], [3.0, 44.0], [13.9, 41.9], [13.9, 41.9]]])
    m = K.patch_mask_ref(kp, 45, 60, 14)
    assert m.shape == (1, 12) and m.sum() == 1 and m[0, 2 * 4 + 0] == 1
    assert K.patch_mask_ref(torch.full((1, 5, 2), -1.0), 45, 60, 14).sum() == 0


# ------------------------------------------------------------------------------------------------ the exact geometry
@pytest.mark.parametrize("g", [2, 3, 5, 9, 17])
def test_dyadic_geometry_is_exact_in_fp32(g):
    """patch = stride = 16, img = 16 g, g - 1 a power of two: gather_coords' own fp32 operations, with and without the fused multiply-add, map
    16 X + 8 + 16 f to X + f exactly for f in quarters (the exactness probes of the GPU tests rest on it)."""
    ax, bx, _, _ = K.gather_consts(16 * g, 16 * g, 16, 16)
    assert ax == 1.0 / (8 * (g - 1)) and bx == -1.0 - 1.0 / (g - 1)
    q = torch.arange(0, 4 * (g - 1) + 1, dtype=torch.float32) / 4                # X + f
    kp = q * 16 + 8
    a, b = torch.tensor(ax), torch.tensor(bx)
    assert a.dtype == torch.float32
    px = kp * torch.tensor(1.0)
    plain = ((a * px + b) + 1.0) * 0.5 * float(g - 1)
    fused = (torch.addcmul(b.double(), a.double(), px.double()).float() + 1.0) * 0.5 * float(g - 1)      # one rounding of a p + b
    assert plain.dtype == torch.float32 and torch.equal(plain, q) and torch.equal(fused, q)
    geom = K.make_geom(g, g, 16)
    kpe, gx, gy = K.exact_keypoints(geom, 2, 50, 5)
    c = K.gather_consts(geom["img_h"], geom["img_w"], 16, 16)
    cx, cy = K.coords64(kpe, 1.0, 1.0, c, g, g)
    assert torch.equal(cx, gx) and torch.equal(cy, gy)


# ------------------------------------------------------------------------------------------------ the probes discriminate
def _taps(gx, gy, gh, gw, clamp_off=0, swap=False):
    """The four-neighbour form of the weights (floor, clamp), split by neighbour row: -> (W through y0, W through y1)."""
    x0, y0 = gx.floor(), gy.floor()
    wx, wy = gx - x0, gy - y0
    if swap:
        wx, wy = wy, wx
    x0, y0 = x0.long(), y0.long()
    x1, y1 = (x0 + 1).clamp(max=gw - 1 - clamp_off), (y0 + 1).clamp(max=gh - 1 - clamp_off)
    B, Nk = gx.shape
    bi, ki = torch.meshgrid(torch.arange(B), torch.arange(Nk), indexing="ij")
    out = []
    for yy, wyy in ((y0, 1 - wy), (y1, wy)):
        Wp = torch.zeros(B, Nk, gh, gw, dtype=F64)
        for xx, wxx in ((x0, 1 - wx), (x1, wx)):
            Wp.index_put_((bi, ki, yy, xx), wyy * wxx, accumulate=True)
        out.append(Wp)
    return out


SEAMS = [(n, False) for n in K.SCATTER_NK] + [(1024, True)]          # True: all 1024 keypoints inside one cell (a full LDS list)


def _worst(wrong, ref, bound):
    err = (wrong - ref).abs()
    r = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(r.max())


@pytest.mark.parametrize("gname", ["generic", "exact", "tiny"])
def test_four_neighbour_form_is_the_hat_form(gname):
    geom = K.GEOMS[gname]
    kp = _kp(geom, 64)
    W, gx, gy = _W(kp, geom)
    a0, a1 = _taps(gx, gy, geom["gh"], geom["gw"])
    assert (a0 + a1 - W).abs().max() < 1e-15


@pytest.mark.parametrize("case", K.FWD_CASES, ids=[c[0] for c in K.FWD_CASES])
def test_wrong_forward_gathers_fail_the_bound(case):
    geom, kp, grids = K.fwd_inputs(case)
    gh, gw = geom["gh"], geom["gw"]
    W, dW = K.geometry64(kp, geom)
    _, gx, gy = _W(kp, geom)
    ref, bound = K.gather_fwd64(grids, W), K.gather_fwd_bound(grids, W, dW)
    assert _worst(ref.float().double(), ref, bound) <= 1.0, "the correctly rounded result is inside the bound"
    wrongs = {"swapped wx / wy": sum(_taps(gx, gy, gh, gw, swap=True))}
    if min(gh, gw) > 2:
        wrongs["neighbour clamp off by one"] = sum(_taps(gx, gy, gh, gw, clamp_off=1))
    for name, Ww in wrongs.items():
        assert _worst(K.gather_fwd64(grids, Ww), ref, bound) >= 8.0, name
    if len(grids) > 1:
        assert _worst(ref * len(grids), ref, bound) >= 8.0, "sum over the grids in place of the mean"


@pytest.mark.parametrize("Nk,full", SEAMS)
def test_wrong_scatters_fail_the_bound(Nk, full):
    for gname in ("exact", "generic"):
        geom, kp, dout = K.scatter_inputs(gname, Nk, 8, full=full)
        gh, gw = geom["gh"], geom["gw"]
        W, dW = K.geometry64(kp, geom)
        _, gx, gy = _W(kp, geom)
        for dtype in (torch.float32, torch.bfloat16):
            ref = K.gather_bwd64(dout, W, 0.25, 1, gw + 1)
            bound = K.gather_bwd_bound(dout, W, dW, 0.25, dtype, False, 1, gw + 1)
            assert _worst(ref.to(dtype).double(), ref, bound) <= 1.0
            a0, _ = _taps(gx, gy, gh, gw)
            assert _worst(K.gather_bwd64(dout, a0, 0.25, 1, gw + 1), ref, bound) >= 8.0, "keypoints dropped from the lines they touch through y1"
            assert _worst(K.gather_bwd64(dout, sum(_taps(gx, gy, gh, gw, swap=True)), 0.25, 1, gw + 1), ref, bound) >= 8.0, "swapped wx / wy"


@pytest.mark.parametrize("Nk,full", SEAMS)
def test_wrong_patch_kernels_fail_the_bound(Nk, full):
    for gname, dtype in (("exact", torch.float32), ("generic", torch.bfloat16)):
        geom, kp, grid, U9 = K.patch_inputs(gname, Nk, 8, dtype, full=full)
        gh, gw = geom["gh"], geom["gw"]
        W, dW = K.geometry64(kp, geom)
        _, gx, gy = _W(kp, geom)
        for od in ((torch.float32, torch.float16) if dtype == torch.float32 else (torch.bfloat16,)):
            ref, bound = K.patch_gather64(grid, W), K.patch_gather_bound(grid, W, dW, od)
            assert _worst(ref.to(od).double(), ref, bound) <= 1.0
            # replicate padding in place of the zero ring
            rep = F.pad(grid.double().permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate").permute(0, 2, 3, 1)
            taps = [K._down(W, rep[:, ky:ky + gh, kx:kx + gw]) for ky in range(3) for kx in range(3)]
            if Nk > 1:                        # (one keypoint inside the grid reads no padding: that list cannot tell, every other one must)
                assert _worst(torch.stack(taps, dim=2).reshape(ref.shape), ref, bound) >= 8.0, "replicate padding"
            assert _worst(K.patch_gather64(grid, sum(_taps(gx, gy, gh, gw, swap=True))), ref, bound) >= 8.0, "swapped wx / wy"
        ref, bound = K.patch_bwd64(U9, W, 1), K.patch_bwd_bound(U9, W, dW, dtype, 1)
        assert _worst(ref.to(dtype).double(), ref, bound) <= 1.0
        # footprint rows y0 - 1 (neighbour row y0 through tap row 0) and y0 + 2 (row y1 through tap row 2) omitted
        a0, a1 = _taps(gx, gy, gh, gw)
        u = U9.double().reshape(2, Nk, 3, 3, -1)
        u0, u1 = u.clone(), u.clone()
        u0[:, :, 0], u1[:, :, 2] = 0, 0
        wrong = K.patch_bwd64(u0.reshape(U9.shape), a0, 1) + K.patch_bwd64(u1.reshape(U9.shape), a1, 1)
        assert _worst(wrong, ref, bound) >= 8.0, "footprint rows y0 - 1 / y0 + 2 omitted"
        full_again = K.patch_bwd64(U9, a0, 1) + K.patch_bwd64(U9, a1, 1)
        assert _worst(full_again, ref, bound) <= 1.0


def test_wrong_references_fail_the_bound_on_the_two_by_two_grid():
    geom, kp, grid, U9 = K.patch_inputs("tiny", K.FWD_NK, 8, torch.float32)
    _, _, dout = K.scatter_inputs("tiny", K.FWD_NK, 8)
    W, dW = K.geometry64(kp, geom)
    _, gx, gy = _W(kp, geom)
    a0, a1 = _taps(gx, gy, 2, 2)
    sw = sum(_taps(gx, gy, 2, 2, swap=True))
    ref, bound = K.gather_bwd64(dout, W, 1.7, 1, 3), K.gather_bwd_bound(dout, W, dW, 1.7, torch.float32, False, 1, 3)
    assert _worst(K.gather_bwd64(dout, a0, 1.7, 1, 3), ref, bound) >= 8.0 and _worst(K.gather_bwd64(dout, sw, 1.7, 1, 3), ref, bound) >= 8.0
    ref, bound = K.patch_gather64(grid, W), K.patch_gather_bound(grid, W, dW, torch.float32)
    rep = F.pad(grid.double().permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate").permute(0, 2, 3, 1)
    taps = [K._down(W, rep[:, ky:ky + 2, kx:kx + 2]) for ky in range(3) for kx in range(3)]
    assert _worst(torch.stack(taps, dim=2).reshape(ref.shape), ref, bound) >= 8.0 and _worst(K.patch_gather64(grid, sw), ref, bound) >= 8.0
    ref, bound = K.patch_bwd64(U9, W, 1), K.patch_bwd_bound(U9, W, dW, torch.float32, 1)
    u = U9.double().reshape(2, K.FWD_NK, 3, 3, -1)
    u0, u1 = u.clone(), u.clone()
    u0[:, :, 0], u1[:, :, 2] = 0, 0
    # (on two lines the rows y0 - 1 / y0 + 2 lie outside the grid for most keypoints: the tap rows dropped here land inside for the rest)
    assert _worst(K.patch_bwd64(U9, sw, 1), ref, bound) >= 8.0
    assert _worst(K.patch_bwd64(u0.reshape(U9.shape), a0, 1) + K.patch_bwd64(u1.reshape(U9.shape), a1, 1), ref, bound) >= 8.0
