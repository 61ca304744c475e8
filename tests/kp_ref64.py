"""fp64 restatements of the keypoint sampling kernels (csrc/elementwise.hip: gd_kp_gather_fwd / _fwd_ln / _bwd / _bwd_det, gd_kp_patch_gather / _h,
gd_kp_patch_bwd_det, gd_kp_depth, gd_patch_mask), the per-element error bounds tests/test_gpu_kp_paths.py holds the kernels to, and the seeded inputs
that file and tests/test_kp_ref_host.py share.  Plain torch, no autograd in a checked formula; every function works on whatever device its inputs
live on.  A test helper, not a test module.

The sampling is stated once, as a dense weight tensor W[B, Nk, gh, gw] = hat(gy - Y) hat(gx - X), hat(t) = max(0, 1 - |t|): bilinear interpolation with
align_corners and border clamp, with no floor and no neighbour index in it.  Every linear kernel of the family is one contraction with W.  hat is
1-Lipschitz, so a kernel whose fp32 coordinate lands on the other side of a cell boundary than the fp64 one is still within the coordinate error of W
at every node: nothing has to be excluded from a comparison.

Notation as in rowwise_ref64: u = 2^-24; an fp32 operation returns the exact result times (1 + d), |d| <= u; a fused multiply-add rounds once, so
counting its product and its sum separately over-counts and stays valid.  First-order bounds carry (1 + 2^-10) for the dropped second-order terms
(which also covers the fp64 roundings of this file, each 2^-29 u).  Layouts: kp [B, Nk, 2] (x, y); a grid is [B, gh, gw, D]."""
import torch
import torch.nn.functional as F

from rowwise_ref64 import SECOND, U, f16_sat, half_ulp  # noqa: F401  (f16_sat, half_ulp: re-exported for the tests)


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ constants and coordinates
def gather_consts(img_h, img_w, patch, stride):
    """(ax, bx, ay, by) exactly as fill_gather forms them: double arithmetic, integer division in (img - patch) / stride, one rounding to fp32.
    k -> a k + b maps the centre of the first patch to -1 and the centre of the last one to +1."""
    half = patch / 2.0
    last_h = ((img_h - patch) // stride) * stride + half
    last_w = ((img_w - patch) // stride) * stride + half
    ay, ax = _f32(2.0 / (last_h - half)), _f32(2.0 / (last_w - half))
    by, bx = _f32(1.0 - last_h * 2.0 / (last_h - half)), _f32(1.0 - last_w * 2.0 / (last_w - half))
    return ax, bx, ay, by


def _axis64(k, s, a, b, g):
    """One axis of gather_coords in fp64 from its fp32 inputs -> (G clamped, bound on |kernel's fp32 G - it|).

    The kernel: p = fl(k s);  t = fl(fl(a p) + b) or one fma;  fl(t + 1);  * 0.5 (exact);  fl(. * (g - 1)).  With P = k s exactly:
        p:        u |P|, carried through a           -> u |a P|
        a p:      u |a P|  (nothing when fused)
        + b:      u |a P + b|
        + 1:      u |a P + b + 1|
    which 0.5 (g - 1) scales, and the last product adds u |G|:
        e_g = 0.5 (g - 1) u (2 |a P| + |a P + b| + |a P + b + 1|) + u |G|
    The clamp to [0, g - 1] is 1-Lipschitz, so e_g holds behind it; where the unclamped G is further outside than e_g, both sides clamp to the same
    end and the bound is ZERO (a far-away or -1-padded keypoint samples the border node exactly)."""
    P = k.double() * s
    t = a * P + b
    G = (t + 1.0) * 0.5 * (g - 1)
    e = (0.5 * (g - 1) * U * (2 * (a * P).abs() + t.abs() + (t + 1.0).abs()) + U * G.abs()) * SECOND
    same_end = (G >= (g - 1) + e) | (G <= -e)
    return G.clamp(0.0, float(g - 1)), torch.where(same_end, torch.zeros_like(e), e)


def coords64(kp, sx, sy, consts, gh, gw):
    """-> (gx, gy) [B, Nk] fp64: grid coordinates of the keypoints from the fp32 constants, clamped to [0, gw - 1] and [0, gh - 1]."""
    ax, bx, ay, by = consts
    return _axis64(kp[..., 0], _f32(sx), ax, bx, gw)[0], _axis64(kp[..., 1], _f32(sy), ay, by, gh)[0]


def coords_bound(kp, sx, sy, consts, gh, gw):
    """-> (e_gx, e_gy) [B, Nk]: see _axis64."""
    ax, bx, ay, by = consts
    return _axis64(kp[..., 0], _f32(sx), ax, bx, gw)[1], _axis64(kp[..., 1], _f32(sy), ay, by, gh)[1]


# ------------------------------------------------------------------------------------------------ the weight tensor
def _hat(g, n):
    """hat(g - X) for the nodes X = 0 .. n - 1 -> [..., n], and |g - X|."""
    d = (g[..., None] - torch.arange(n, dtype=torch.float64, device=g.device)).abs()
    return (1.0 - d).clamp_min(0.0), d


def weights64(gx, gy, gh, gw):
    """W[B, Nk, gh, gw] = hat(gy - Y) hat(gx - X)."""
    return _hat(gy, gh)[0][..., :, None] * _hat(gx, gw)[0][..., None, :]


def weights_bound(gx, gy, ex, ey, gh, gw):
    """dW[B, Nk, gh, gw] >= |the weight a kernel gives node (Y, X) - W|.

    A kernel's x factor at node X is fl(1 - wx) (X = x0) or wx (X = x1), wx = G - floor(G) exact: hat(G_kernel - X) (1 + d).  hat is 1-Lipschitz:
        d_x = e_gx + u (hat_x + e_gx)        where |gx - X| < 1 + e_gx  (a node either side can reach), else 0: both are exactly 0
    and likewise d_y.  The product of the two factors rounds once more:
        |dW| <= d_y hat_x + hat_y d_x + d_y d_x + u (hat_y + d_y) (hat_x + d_x)
    d_y d_x is kept: where the fp64 keypoint sits ON a node and the fp32 one a hair to its lower left, the diagonal neighbour gets e_gx e_gy and W
    has nothing there.  A weight folded with further factors (1 / ngrid, scale) rounds again; the callers count those in n_add."""
    hx, ax = _hat(gx, gw)
    hy, ay = _hat(gy, gh)
    dx = torch.where(ax < 1.0 + ex[..., None], ex[..., None] + U * (hx + ex[..., None]), torch.zeros_like(hx))
    dy = torch.where(ay < 1.0 + ey[..., None], ey[..., None] + U * (hy + ey[..., None]), torch.zeros_like(hy))
    hx, hy, dx, dy = hx[..., None, :], hy[..., :, None], dx[..., None, :], dy[..., :, None]
    return dy * hx + hy * dx + dy * dx + U * (hy + dy) * (hx + dx)


def geometry64(kp, geom):
    """-> (W, dW) of keypoints kp under geom = dict(gh, gw, patch, stride, img_h, img_w, sx, sy)."""
    c = gather_consts(geom["img_h"], geom["img_w"], geom["patch"], geom["stride"])
    gh, gw = geom["gh"], geom["gw"]
    gx, gy = coords64(kp, geom["sx"], geom["sy"], c, gh, gw)
    ex, ey = coords_bound(kp, geom["sx"], geom["sy"], c, gh, gw)
    return weights64(gx, gy, gh, gw), weights_bound(gx, gy, ex, ey, gh, gw)


def _down(W, v):          # [B, Nk, gh, gw] x [B, gh, gw, D] -> [B, Nk, D]
    return torch.einsum("bkyx,byxd->bkd", W, v)


def _up(W, v):            # [B, Nk, gh, gw] x [B, Nk, D] -> [B, gh, gw, D]
    return torch.einsum("bkyx,bkd->byxd", W, v)


def embed(dense, prefix, pitch):
    """[B, gh, gw, D] -> the token layout [B, prefix + gh pitch, D]: prefix rows and the separator columns x >= gw zero."""
    B, gh, gw, D = dense.shape
    out = torch.zeros(B, prefix + gh * pitch, D, dtype=dense.dtype, device=dense.device)
    out[:, prefix:].view(B, gh, pitch, D)[:, :, :gw] = dense
    return out


def _store(ref, b, dtype):
    """A bound b on the fp32 value, behind one store in `dtype` (fp16 saturates: compare against the reference clamped to +-65504)."""
    if dtype == torch.float32:
        return b
    mag = ref.abs() + b
    if dtype == torch.float16:
        mag = mag.clamp(max=65504.0)
    return b + half_ulp(mag, dtype)


# ------------------------------------------------------------------------------------------------ forward gathers
def gather_fwd64(grids, W):
    """gd_kp_gather_fwd: the mean over the grids of their samples -> [B, Nk, D] fp64."""
    return sum(_down(W, g.double()) for g in grids) / len(grids)


def gather_fwd_bound(grids, W, dW):
    """acc += w00 v00 + w01 v01 + w10 v10 + w11 v11 per grid, then acc fl(1 / ngrid): a term passes its product, at most 4 ngrid additions, the
    constant's rounding and the last product: n_add = 4 ngrid + 3.  The output is fp32 whatever the grid's type (its values are read exactly)."""
    n = 4 * len(grids) + 3
    b = sum(_down(dW, g.double().abs()) + n * U * _down(W + dW, g.double().abs()) for g in grids)
    return b / len(grids) * SECOND


def gather_ln_fwd64(grids, means, rstds, gamma, beta, W):
    """gd_kp_gather_fwd_ln: the grids normalised in fp64 from the kernel's own inputs (means / rstds [B, gh, gw] fp32), then gathered."""
    normed = [(g.double() - m.double()[..., None]) * r.double()[..., None] * gamma.double() + beta.double() for g, m, r in zip(grids, means, rstds)]
    return gather_fwd64(normed, W)


def gather_ln_fwd_bound(grids, means, rstds, gamma, beta, W, dW):
    """The kernel folds a = fl(w rstd) per tap, sums a x over the four taps, subtracts sub = sum a mu, accumulates over the grids, multiplies by
    fl(1 / ngrid) and ends in fma(., gamma, beta).  The same a multiplies x and mu, so the weight's error meets rstd |x - mu|; the roundings meet
    |x| and |mu| SEPARATELY (the subtraction comes after the sums: rows of large mean pay for it).  A product a x passes the rounding of a, its own,
    3 additions, the subtraction, ngrid accumulations, the constant and the last product: n_add = ngrid + 8.
        inner = (1 / ngrid) sum_t [ contract(dW, rstd |x - mu|) + (ngrid + 8) u contract(W + dW, rstd (|x| + |mu|)) ]
        |d out| <= |gamma| inner + u (|out| + |gamma| inner)"""
    n = len(grids) + 8
    inner = 0
    for g, m, r in zip(grids, means, rstds):
        x, mu, rs = g.double(), m.double()[..., None], r.double().abs()[..., None]
        inner = inner + _down(dW, rs * (x - mu).abs()) + n * U * _down(W + dW, rs * (x.abs() + mu.abs()))
    inner = inner / len(grids) * gamma.double().abs()
    ref = gather_ln_fwd64(grids, means, rstds, gamma, beta, W)
    return (inner + U * (ref.abs() + inner)) * SECOND


# ------------------------------------------------------------------------------------------------ scatters (the gathers' transposes)
def gather_bwd64(dout, W, scale, prefix=0, pitch=None):
    """gd_kp_gather_bwd (scale = 1 / ngrid) / gd_kp_gather_bwd_det: [B, prefix + gh pitch, D] fp64, prefix rows and separator columns zero."""
    return embed(_up(W, dout.double()) * scale, prefix, W.shape[-1] if pitch is None else pitch)


def gather_bwd_bound(dout, W, dW, scale, out_dtype, atomic, prefix=0, pitch=None):
    """cnt = keypoints that can reach the cell (W + dW > 0).  Deterministic kernel: the cell adds, in list order, one w g per listed keypoint that
    touches it (an addend of exactly 0 changes nothing); w carries the product with scale: n_add = cnt + 3.  Atomic kernel: four atomicAdd per
    keypoint, in any order — up to 4 cnt additions on one cell (clamped neighbours coincide), w carries fl(1 / ngrid) and its product:
    n_add = 4 cnt + 3.  Any order of n additions costs each term at most n u.  Then one store (bf16: half_ulp).  Where no keypoint reaches, and
    in the prefix rows and separator columns, the bound is ZERO."""
    a = dout.double().abs()
    cnt = ((W + dW) > 0).double().sum(1)[..., None]
    n = (4 * cnt if atomic else cnt) + 3
    b = (_up(dW, a) + n * U * _up(W + dW, a)) * abs(scale) * SECOND
    pt = W.shape[-1] if pitch is None else pitch
    return _store(gather_bwd64(dout, W, scale, prefix, pitch), embed(b, prefix, pt), out_dtype)


# ------------------------------------------------------------------------------------------------ 3x3 patches at the keypoints
def _pad1(grid):
    B, gh, gw, D = grid.shape
    pad = torch.zeros(B, gh + 2, gw + 2, D, dtype=torch.float64, device=grid.device)
    pad[:, 1:gh + 1, 1:gw + 1] = grid.double()
    return pad


def patch_gather64(grid, W):
    """gd_kp_patch_gather(_h): out[(b, k), (ky, kx, c)] = sum_{Y, X} W[b, k, Y, X] grid0[b, Y + ky - 1, X + kx - 1, c], grid0 = the grid inside one
    ring of zeros (conv padding 1) -> [B Nk, 9 D] fp64."""
    B, gh, gw, D = grid.shape
    pad = _pad1(grid)
    taps = [_down(W, pad[:, ky:ky + gh, kx:kx + gw]) for ky in range(3) for kx in range(3)]
    return torch.stack(taps, dim=2).reshape(B * W.shape[1], 9 * D)


def patch_gather_bound(grid, W, dW, out_dtype):
    """Each tap: four products, three additions -> n_add = 4; one store in out_dtype (fp16: against patch_gather64 clamped to +-65504)."""
    B, gh, gw, D = grid.shape
    pad = _pad1(grid).abs()
    taps = [_down(dW, pad[:, ky:ky + gh, kx:kx + gw]) + 4 * U * _down(W + dW, pad[:, ky:ky + gh, kx:kx + gw]) for ky in range(3) for kx in range(3)]
    b = torch.stack(taps, dim=2).reshape(B * W.shape[1], 9 * D) * SECOND
    return _store(patch_gather64(grid, W), b, out_dtype)


def _patch_up(W, U9, gh, gw):
    B, Nk = W.shape[:2]
    D = U9.shape[-1] // 9
    u = U9.reshape(B, Nk, 3, 3, D)
    pad = torch.zeros(B, gh + 2, gw + 2, D, dtype=torch.float64, device=W.device)
    for ky in range(3):
        for kx in range(3):
            pad[:, ky:ky + gh, kx:kx + gw] += _up(W, u[:, :, ky, kx])
    return pad[:, 1:gh + 1, 1:gw + 1]


def patch_bwd64(U9, W, prefix=0):
    """gd_kp_patch_bwd_det: the exact transpose of patch_gather64.  U9 [B Nk, 9 D] -> tokens [B, prefix + gh gw, D] fp64, prefix rows zero."""
    gh, gw = W.shape[-2:]
    return embed(_patch_up(W, U9.double(), gh, gw), prefix, gw)


def patch_bwd_bound(U9, W, dW, out_dtype, prefix=0):
    """A token adds, in list order, one term w_ab u per (keypoint, neighbour) whose tap lands on it — cnt of them, the neighbours that W + dW can
    reach counted through all nine taps: n_add = cnt + 1 (the product; the weight's own product is in dW), then one store."""
    gh, gw = W.shape[-2:]
    a = U9.double().abs()
    ones = torch.ones(a.shape[0], 9, dtype=torch.float64, device=a.device)
    cnt = _patch_up(((W + dW) > 0).double(), ones, gh, gw)
    b = (_patch_up(dW, a, gh, gw) + (cnt + 1) * U * _patch_up(W + dW, a, gh, gw)) * SECOND
    return _store(patch_bwd64(U9, W, prefix), embed(b, prefix, gw), out_dtype)


# ------------------------------------------------------------------------------------------------ depth at keypoints, patch mask
def _depth_lin(kp, H, W):
    lin = (kp[..., 1].float() * float(W) + kp[..., 0].float()).long()          # fp32 y W + x (one rounding each), truncated toward zero
    return lin.clamp(0, H * W - 1)


def _window_mean(d, lin):
    B, H, W = d.shape
    m = F.avg_pool2d(F.pad(d[:, None], (1, 1, 1, 1), mode="replicate"), 3, stride=1).reshape(B, H * W)
    return m.gather(1, lin)


def kp_depth64(depth, kp):
    """gd_kp_depth: the fp32 (y W + x) truncated to an integer and clamped into the image, as the kernel and the reference project do, then the 3x3
    replicate-padded mean in fp64.  depth [B, H, W], kp [B, Nk, 2] -> [B, Nk].  (The kernel may fuse y W + x; the tests keep y W exact in fp32.)"""
    return _window_mean(depth.double(), _depth_lin(kp, *depth.shape[1:]))


def kp_depth_bound(depth, kp):
    """Eight additions of positive-or-not terms and the division by 9 (a rounded reciprocal and a product at worst): ten roundings of the mean
    magnitude of the window."""
    return 10 * U * _window_mean(depth.double().abs(), _depth_lin(kp, *depth.shape[1:]))


def patch_mask_ref(kp, H, W, P):
    """gd_patch_mask: uint8 [B, (H // P) (W // P)], 1 where a keypoint with 0 <= x < W, 0 <= y < H falls into the patch (int(y) // P, int(x) // P).
    A keypoint in the remainder strip (H or W no multiple of P) has no patch and marks nothing."""
    B = kp.shape[0]
    ph, pw = H // P, W // P
    x, y = kp[..., 0].float(), kp[..., 1].float()
    xi, yi = x.long() // P, y.long() // P
    ok = (x >= 0) & (x < W) & (y >= 0) & (y < H) & (xi < pw) & (yi < ph)
    mask = torch.zeros(B, ph * pw, dtype=torch.uint8, device=kp.device)
    for b in range(B):
        mask[b, (yi[b] * pw + xi[b])[ok[b]]] = 1
    return mask


# ------------------------------------------------------------------------------------------------ the shared inputs
def make_geom(gh, gw, patch, sx=1.0, sy=1.0):
    return dict(gh=gh, gw=gw, patch=patch, stride=patch, img_h=gh * patch, img_w=gw * patch, sx=_f32(sx), sy=_f32(sy))


GEOMS = {
    "exact": make_geom(5, 9, 16),                     # gh - 1 = 4, gw - 1 = 8: dyadic constants, see exact_keypoints
    "generic": make_geom(6, 7, 14, sx=1.3, sy=0.7),
    "tiny": make_geom(2, 2, 16),
}


def to_pixels(gx, gy, geom):
    """Grid coordinates -> keypoints (source-frame pixels): node X sits at the patch centre stride X + patch / 2 of the model frame."""
    P, S = geom["patch"], geom["stride"]
    x = (gx.double() * S + P / 2.0) / geom["sx"]
    y = (gy.double() * S + P / 2.0) / geom["sy"]
    return torch.stack([x, y], -1).float()


def _specials(geom):
    gh, gw = geom["gh"], geom["gw"]
    X1, Y1, Xm, Ym = min(1, gw - 1), min(1, gh - 1), max(gw - 2, 0), max(gh - 2, 0)
    nodes = [(0, 0), (gw - 1, gh - 1), (0, gh - 1), (gw - 1, 0), (X1, Y1), (Xm, Ym), (gw - 1, Y1), (X1, gh - 1), (X1, 0), (0, Ym)]
    mids = [(0.5, 0.5), (Xm + 0.5, Ym + 0.5), (0.5, Ym + 0.5), (Xm + 0.5, 0.5), (X1 * 0.5 + Xm * 0.5, Y1), (X1, Ym + 0.5)]
    g = torch.tensor(nodes + mids, dtype=torch.float64)
    kp = to_pixels(g[:, 0], g[:, 1], geom)
    inf = torch.tensor(float("inf"))
    ulps = []
    for i in (4, 5, 1, 0):                            # one fp32 ulp either side of a node, in x, in y, in both
        for sgn in (-1.0, 1.0):
            ulps += [torch.stack([torch.nextafter(kp[i, 0], sgn * inf), kp[i, 1]]), torch.stack([kp[i, 0], torch.nextafter(kp[i, 1], sgn * inf)]),
                     torch.nextafter(kp[i], sgn * inf)]
    sx, sy, h, w = geom["sx"], geom["sy"], geom["img_h"], geom["img_w"]
    raw = torch.tensor([[0.0, 0.0], [(w - 1) / sx, (h - 1) / sy],                                           # the image's corners
                        [-1000.0, h / (2 * sy)], [1e4, h / (2 * sy)], [w / (2 * sx), -1000.0], [w / (2 * sx), 1e4],   # far outside, each side
                        [-1.0, -1.0]])                                                                      # the loaders' padding
    return torch.cat([raw.float(), kp, torch.stack(ulps)])


def probe_keypoints(geom, B, Nk, seed):
    """[B, Nk, 2] fp32: the image's and the grid's corners, far outside on each side, the -1 padding, exact nodes (every corner and edge cell), cell
    midpoints, one fp32 ulp either side of nodes — then random ones from 0.7 cells outside the grid inwards.  Row b starts 5 b into the list of
    specials; rows after the first end in -1 padding."""
    g = torch.Generator().manual_seed(seed)
    sp = _specials(geom)
    gh, gw = geom["gh"], geom["gw"]
    out = []
    for b in range(B):
        rx = torch.rand(Nk, generator=g, dtype=torch.float64) * (gw + 0.4) - 0.7
        ry = torch.rand(Nk, generator=g, dtype=torch.float64) * (gh + 0.4) - 0.7
        rx[0], ry[0] = (rx[0] + 0.7) * (gw - 1) / (gw + 0.4), (ry[0] + 0.7) * (gh - 1) / (gh + 0.4)      # the first one inside the grid
        kp = to_pixels(rx, ry, geom)
        s = sp.roll(-5 * b, 0)[:Nk if Nk >= 32 else Nk // 2]          # a short list keeps random keypoints too
        kp[:s.shape[0]] = s
        if b > 0 and Nk > 1:
            kp[Nk - max(1, Nk // 8):] = -1.0
        out.append(kp)
    return torch.stack(out)


def exact_keypoints(geom, B, Nk, seed):
    """Keypoints of the exact geometry (patch = stride = 16, sx = sy = 1, g - 1 a power of two) at grid coordinates in quarters, nodes and the far
    corner included: 16 X + 8 + 16 f maps to X + f with no rounding at all in fp32 -> (kp [B, Nk, 2], gx, gy) with gx, gy the exact coordinates."""
    g = torch.Generator().manual_seed(seed)
    gx = torch.randint(0, 4 * (geom["gw"] - 1) + 1, (B, Nk), generator=g).double() / 4
    gy = torch.randint(0, 4 * (geom["gh"] - 1) + 1, (B, Nk), generator=g).double() / 4
    gx[:, 0], gy[:, 0] = geom["gw"] - 1, geom["gh"] - 1
    return to_pixels(gx, gy, geom), gx, gy


def line_keypoints(geom, B, Nk, X, Y, seed):
    """Every keypoint strictly inside cell (Y, X): all Nk of them are on the lists of lines Y and Y + 1 (a full LDS list at Nk = 1024) and of the
    column pair X, X + 1."""
    g = torch.Generator().manual_seed(seed)
    fx = 0.05 + 0.9 * torch.rand(B, Nk, generator=g, dtype=torch.float64)
    fy = 0.05 + 0.9 * torch.rand(B, Nk, generator=g, dtype=torch.float64)
    return to_pixels(X + fx, Y + fy, geom)


def cover_grid(geom, B, D, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, geom["gh"], geom["gw"], D, generator=g) * scale


# The cases of tests/test_gpu_kp_paths.py; tests/test_kp_ref_host.py checks on the CPU that wrong references fail the bounds AT THESE INPUTS.
#            name            geometry   grid dtype      D     ngrid pitch+ prefix misaligned
FWD_CASES = [("f32_vec8", "generic", torch.float32, 8, 1, 0, 0, None),
             ("f32_vec1032", "exact", torch.float32, 1032, 2, 1, 1, None),           # second trip of the channel loop (128 threads x 4 channels)
             ("bf16_vec8", "generic", torch.bfloat16, 8, 3, 1, 0, None),
             ("bf16_vec1032", "exact", torch.bfloat16, 1032, 4, 0, 1, None),
             ("f32_scalar6", "generic", torch.float32, 6, 4, 0, 1, None),
             ("bf16_scalar4", "exact", torch.bfloat16, 4, 2, 1, 0, None),
             ("f32_misaligned_grid", "generic", torch.float32, 8, 2, 0, 0, "grid"),
             ("bf16_misaligned_grid", "exact", torch.bfloat16, 8, 2, 1, 1, "grid"),
             ("f32_misaligned_out", "generic", torch.float32, 8, 1, 1, 1, "out"),
             ("f16_8", "generic", torch.float16, 8, 2, 0, 1, None),
             ("f16_6", "exact", torch.float16, 6, 1, 1, 0, None),
             ("f32_tiny", "tiny", torch.float32, 8, 3, 1, 1, None),
             ("bf16_tiny", "tiny", torch.bfloat16, 4, 1, 0, 0, None)]
FWD_NK = 48
SCATTER_NK = [1, 63, 64, 65, 256, 257, 1024]          # the wave-ballot seam (64) and the 256-wide scan seam, either side; the LDS list's capacity


def fwd_inputs(case, seed=11):
    """-> (geom, kp [2, FWD_NK, 2], grids: ngrid x [2, gh, gw, D] in the case's dtype)."""
    name, gname, dtype, D, ngrid = case[:5]
    geom = GEOMS[gname]
    kp = probe_keypoints(geom, 2, FWD_NK, seed)
    return geom, kp, [cover_grid(geom, 2, D, seed * 16 + t + 1).to(dtype) for t in range(ngrid)]


def scatter_inputs(gname, Nk, D, seed=23, full=False):
    """-> (geom, kp [2, Nk, 2], dout [2, Nk, D] fp32); full: every keypoint inside one cell (line_keypoints)."""
    geom = GEOMS[gname]
    kp = line_keypoints(geom, 2, Nk, geom["gw"] - 2, 1, seed) if full else probe_keypoints(geom, 2, Nk, seed)
    g = torch.Generator().manual_seed(seed + 1)
    return geom, kp, torch.randn(2, Nk, D, generator=g)


def patch_inputs(gname, Nk, D, dtype, seed=37, full=False):
    """-> (geom, kp [2, Nk, 2], grid [2, gh, gw, D] in dtype, U9 [2 Nk, 9 D] in dtype)."""
    geom, kp, _ = scatter_inputs(gname, Nk, 8, seed, full)
    g = torch.Generator().manual_seed(seed + 2)
    return geom, kp, cover_grid(geom, 2, D, seed + 3).to(dtype), torch.randn(2 * Nk, 9 * D, generator=g).to(dtype)
