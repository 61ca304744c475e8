"""GPU: the correspondence-evaluation kernels (gd_match_argmax, gd_transfer_argmax) against fp64 CPU restatements, and the
end-to-end semantic transfer of gd_amd.evaluate against the oracle's ViT forward."""
import pytest
import torch
import torch.nn.functional as F

import gd_amd  # noqa: F401
import gd_oracle as O
from gd_amd import evaluate as E
from gd_amd import ops

pytestmark = pytest.mark.gpu

U16, U32 = 2.0 ** -11, 2.0 ** -24


def _data(M, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, D, generator=g), torch.randn(N, D, generator=g)


def _check_direction(S, absS, pick, precision, D):
    """S, absS [R, C] fp64 (scores, sum |a_k b_k|); pick [R] the kernel's argmax per row."""
    R = S.shape[0]
    rows = torch.arange(R)
    best, ref = S.max(dim=1)
    ref = S.argmax(dim=1)           # first occurrence
    err = (2 * U16 + D * U32 if precision == "f16" else D * U32) * absS     # operand rounding + fp32 accumulation, per entry
    bound = err[rows, pick] + err[rows, ref]
    got = S[rows, pick]
    assert bool((got >= best - bound).all()), float((best - got - bound).max())
    if precision == "f32":
        second = S.clone()
        second[rows, ref] = -float("inf")
        gap = best - second.max(dim=1).values
        sure = gap > bound
        assert torch.equal(pick[sure], ref[sure])


CASES = [(1, 5000, 8), (127, 129, 24), (129, 127, 768), (1000, 1000, 1024), (5000, 1, 24), (5000, 127, 8), (1, 1, 1024),
         (129, 1000, 8), (1000, 5000, 768)]


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("M,N,D", CASES)
def test_match_argmax_vs_fp64(M, N, D, precision):
    a, b = _data(M, N, D, seed=M * 7 + N * 3 + D)
    r = ops.match_argmax(a.cuda(), b.cuda(), both=True, precision=precision, want_scores=True, want_mutual=True)
    row, col, mut = r.row_idx.cpu(), r.col_idx.cpu(), r.mutual.cpu()
    assert row.dtype == torch.int64 and row.shape == (M,) and col.shape == (N,)
    assert int(row.min()) >= 0 and int(row.max()) < N and int(col.min()) >= 0 and int(col.max()) < M
    A, B = a.double(), b.double()
    S, absS = A @ B.T, A.abs() @ B.abs().T
    _check_direction(S, absS, row, precision, D)
    _check_direction(S.T, absS.T, col, precision, D)
    assert torch.equal(mut, col[row] == torch.arange(M))
    # the scores are the maxima (unscaled in f16 mode)
    tol = (2 * U16 + D * U32 if precision == "f16" else D * U32) * 2
    assert torch.allclose(r.row_score.cpu().double(), S.max(dim=1).values, rtol=0, atol=float(tol * absS.max()) + 1e-6)


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_match_argmax_ties_pick_the_smallest_index_and_runs_repeat(precision):
    torch.manual_seed(3)
    M, N, D = 300, 520, 64
    a = F.normalize(torch.randn(M, D), dim=1)
    b = F.normalize(torch.randn(N, D), dim=1)
    b[200], b[450], b[451] = b[50], b[50], b[50]       # exact duplicate columns; row 7 of a IS that vector
    a[7] = b[50]
    a[150], a[299] = a[20], a[20]                      # exact duplicate rows; column 5 of b IS that vector
    b[5] = a[20]
    r1 = ops.match_argmax(a.cuda(), b.cuda(), precision=precision, want_scores=True, want_mutual=True)
    r2 = ops.match_argmax(a.cuda(), b.cuda(), precision=precision, want_scores=True, want_mutual=True)
    assert int(r1.row_idx[7]) == 50
    assert int(r1.col_idx[5]) == 20
    for f in ("row_idx", "col_idx", "mutual", "row_score", "col_score"):
        assert torch.equal(getattr(r1, f), getattr(r2, f)), f
    # one direction only: the same rows
    r3 = ops.match_argmax(a.cuda(), b.cuda(), both=False, precision=precision)
    assert r3.col_idx is None and torch.equal(r3.row_idx, r1.row_idx)


def test_match_argmax_large_grid_subset():
    """N > 65536 and M * N > 2^31 (64-bit offsets, a grid of 140k tiles), checked on random rows and columns."""
    M, N, D = 32768, 70000, 64
    assert M * N > 2 ** 31
    g = torch.Generator(device="cuda").manual_seed(11)
    a = torch.randn(M, D, device="cuda", generator=g)
    b = torch.randn(N, D, device="cuda", generator=g)
    sel = torch.randperm(M, generator=torch.Generator().manual_seed(1))[:200]
    selc = torch.randperm(N, generator=torch.Generator().manual_seed(2))[:200]
    sel = torch.cat([sel, torch.tensor([0, M - 1])])
    selc = torch.cat([selc, torch.tensor([0, N - 1])])
    A, B = a.cpu().double(), b.cpu().double()
    for precision in ("f32", "f16"):
        r = ops.match_argmax(a, b, precision=precision, want_mutual=True)
        row, col = r.row_idx.cpu(), r.col_idx.cpu()
        _check_direction(A[sel] @ B.T, A[sel].abs() @ B.abs().T, row[sel], precision, D)
        _check_direction(B[selc] @ A.T, B[selc].abs() @ A.abs().T, col[selc], precision, D)
        assert torch.equal(r.mutual.cpu(), col[row] == torch.arange(M))


def test_mutual_nearest_neighbours():
    torch.manual_seed(5)
    t = F.normalize(torch.randn(3000, 256), dim=1)
    d = F.normalize(t[torch.randperm(3000)[:700]] + 0.05 * torch.randn(700, 256), dim=1)
    nbr1, nbr2, m = E.mutual_nearest_neighbours(d.cuda(), t.cuda(), precision="f32")
    S = d.double() @ t.double().T
    assert torch.equal(nbr1.cpu(), S.argmax(1))                     # every query's source template wins by a wide margin
    _check_direction(S.T, t.double().abs() @ d.double().abs().T, nbr2.cpu(), "f32", 256)
    assert torch.equal(m.cpu(), nbr2.cpu()[nbr1.cpu()] == torch.arange(700))
    assert int(m.sum()) > 600


# ------------------------------------------------------------------------------------------------------------ transfer argmax
def _field_fp64(T, q, img_h, img_w, patch, stride):
    """The reference's materialising pipeline in fp64: T [D, gh, gw] -> interpolate -> edge pad -> einsum with q [K, D] -> [K, H*W]."""
    g = E.transfer_geometry(img_h, img_w, patch, stride)
    up = F.interpolate(T.double()[None], size=(g["ds_h"], g["ds_w"]), mode="bilinear", align_corners=True)
    up = F.pad(up, (g["left"], g["right"], g["top"], g["bottom"]), mode="replicate")[0]
    return torch.einsum("kd,dp->kp", q.double(), up.reshape(up.shape[0], -1))


def _transfer_check(T, q, img_h, img_w, patch, stride):
    S = torch.einsum("kd,dhw->khw", q.double(), T.double()).float()
    xy = ops.transfer_argmax(S.cuda(), (img_h, img_w), patch, stride).cpu()
    fld = _field_fp64(T, q, img_h, img_w, patch, stride)
    best = fld.max(dim=1).values
    ref = fld.argmax(dim=1)
    pick = xy[:, 1] * img_w + xy[:, 0]
    tol = 1e-5 * float(fld.abs().max())
    assert bool((fld[torch.arange(len(pick)), pick] >= best - tol).all())
    below = torch.where(fld < best[:, None], fld, torch.full_like(fld, -float("inf")))      # plateau copies of the max are not a gap
    sure = best - below.max(dim=1).values > tol
    assert int(sure.sum()) >= len(pick) // 2
    assert torch.equal(pick[sure], ref[sure])
    return xy


@pytest.mark.parametrize("img_h,img_w,patch,stride", [(640, 640, 16, 16), (640, 640, 14, 7), (480, 640, 16, 16), (203, 157, 14, 14)])
def test_transfer_argmax_vs_materialised_field(img_h, img_w, patch, stride):
    gh, gw = E.token_grid(img_h, img_w, patch, stride)
    g = torch.Generator().manual_seed(img_h + patch)
    T = torch.randn(32, gh, gw, generator=g)
    q = F.normalize(torch.randn(12, 32, generator=g), dim=1)
    _transfer_check(T, q, img_h, img_w, patch, stride)


def test_transfer_argmax_border_nodes():
    """Maxima on border nodes: the edge padding makes a plateau, and the raster-first pixel of it must come back exactly."""
    H = W = 640
    gh = gw = 40
    S = torch.randn(4, gh, gw, generator=torch.Generator().manual_seed(0))
    S[0, 0, 0] = 50.0               # top-left corner: the whole 9 x 9 top-left block is the plateau -> pixel (0, 0)
    S[1, gh - 1, 3] = 50.0          # bottom edge node: plateau runs down the bottom pad from the node's row
    S[2, 17, gw - 1] = 50.0         # right edge node: plateau runs along the right pad
    S[3, 0, 21] = 50.0              # top edge node: first occurrence is in row 0
    xy = ops.transfer_argmax(S.cuda(), (H, W), 16, 16).cpu().tolist()
    # node (i, j) sits at pixel (8 + 16 j, 8 + 16 i)
    assert xy[0] == [0, 0]
    assert xy[1] == [8 + 16 * 3, 8 + 16 * (gh - 1)]
    assert xy[2] == [8 + 16 * (gw - 1), 8 + 16 * 17]
    assert xy[3] == [8 + 16 * 21, 0]
    for k in range(4):              # the same picks from the materialised field (interpolate -> edge pad -> first argmax)
        up = F.interpolate(S[k][None, None].double(), size=(625, 625), mode="bilinear", align_corners=True)
        up = F.pad(up, (8, 7, 8, 7), mode="replicate").reshape(-1)
        idx = int(up.argmax())
        assert xy[k] == [idx % W, idx // W]


# ------------------------------------------------------------------------------------------------------------ end to end
def _tiny_engine(img):
    from gd_amd.finetune import FinetuneGD
    torch.manual_seed(0)
    eng = FinetuneGD(r=4, backbone="vit_tiny_test", patch_size=16, img_size=img, variant="vggt", geometry="shared", dtype="f32",
                     lora_b_std=0.05, vit_kwargs=dict(init_values=1.0), teacher_patch=16).cuda()
    return eng.eval()


def _oracle_grid(eng, img, p, tr, refine, cfg):
    x = O.normalize_image(img[None], cfg["mean"], cfg["std"])
    _, last = O.vit_forward(x, p, cfg, tr)
    tok = O.final_norm(last, p, cfg)[:, 1:]
    gh = gw = img.shape[-1] // 16
    grid = tok.reshape(1, gh, gw, -1).permute(0, 3, 1, 2)
    return F.conv2d(grid.double(), refine["weight"].double(), refine["bias"].double(), padding=1)[0]      # [D, gh, gw]


def test_transfer_keypoints_and_pck_end_to_end():
    from gd_amd.synthetic import export_params
    img_size = 640
    eng = _tiny_engine(img_size)
    p, tr, refine, _, cfg = export_params(eng)
    g = torch.Generator().manual_seed(4)
    base = F.interpolate(torch.rand(1, 3, 40, 40, generator=g), size=(img_size, img_size), mode="bilinear", align_corners=False)[0]
    img1 = base.clone()
    img2 = torch.roll(base, shifts=(32, 48), dims=(1, 2))
    K = 16
    kps1 = torch.cat([torch.randint(40, 560, (K, 2), generator=g).float(), torch.ones(K, 1)], 1)
    kps2 = kps1.clone()
    kps2[:, 0] += 48
    kps2[:, 1] += 32
    kps2[::5, 2] = 0
    xy = E.transfer_keypoints(eng, img1.cuda(), img2.cuda(), kps1.cuda(), img_size=img_size).cpu()
    assert xy.shape == (K, 2) and xy.dtype == torch.int64
    # CPU restatement on the oracle's forward: queries with the reference's patch-14 mapping, the materialised field, argmax
    T1, T2 = _oracle_grid(eng, img1, p, tr, refine, cfg), _oracle_grid(eng, img2, p, tr, refine, cfg)
    q = O.interpolate_features(T1[None], kps1[None, :, :2].double(), img_size, img_size, normalize=True)[0].T     # [K, D], p14 default
    fld = _field_fp64(T2, q, img_size, img_size, 16, 16)
    best, ref = fld.max(dim=1).values, fld.argmax(dim=1)
    pick = xy[:, 1] * img_size + xy[:, 0]
    tol = 2e-4 * float(fld.abs().max())
    assert bool((fld[torch.arange(K), pick] >= best - tol).all())
    below = torch.where(fld < best[:, None], fld, torch.full_like(fld, -float("inf")))
    sure = best - below.max(dim=1).values > tol
    assert torch.equal(pick[sure], ref[sure])
    # PCK over the pair(s): the formula on the transferred points, and the restatement's whenever every pick was sure
    res = E.semantic_transfer_pck(eng, [(img1.cuda(), img2.cuda(), kps1, kps2)] * 2, img_size=img_size)
    vis = kps1[:, 2] * kps2[:, 2] > 0
    want = E.pck(torch.cat([xy[vis][:, [1, 0]]] * 2), torch.cat([kps2[vis][:, [1, 0]]] * 2), img_size)
    assert res["n"] == 2 * int(vis.sum())
    assert [res["PCK0.10"], res["PCK0.05"], res["PCK0.15"]] == want.tolist()
    if bool(sure.all()):
        refxy = torch.stack([ref % img_size, ref // img_size], 1)
        assert want.tolist() == E.pck(torch.cat([refxy[vis][:, [1, 0]]] * 2), torch.cat([kps2[vis][:, [1, 0]]] * 2), img_size).tolist()


def test_descriptors_at_matches_the_oracle():
    from gd_amd.synthetic import export_params
    eng = _tiny_engine(128)
    p, tr, refine, _, cfg = export_params(eng)
    img = torch.rand(3, 128, 128, generator=torch.Generator().manual_seed(9))
    pts = torch.rand(20, 2, generator=torch.Generator().manual_seed(10)) * 127
    got = E.descriptors_at(eng, img.cuda(), pts.cuda(), patch_size=16, stride=16, normalize=True).cpu()
    T = _oracle_grid(eng, img, p, tr, refine, cfg)
    want = O.interpolate_features(T[None], pts[None].double(), 128, 128, normalize=True, patch_size=16, stride=16)[0].T
    assert got.shape == (20, T.shape[0])
    assert float((got.double() - want).abs().max()) < 2e-4
