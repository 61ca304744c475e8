"""Correspondence evaluation of a fine-tuned backbone: the two methods the reference's EvaluationCallback runs every 10 epochs
(src/evaluate_timm.py:591-730) — semantic keypoint transfer (:461-588) and the OnePose++ descriptor matching (:140-179) — with
the features on the HIP forward and the matching on gd_match_argmax / gd_transfer_argmax.  Everything runs under
torch.no_grad(); nothing here touches the training step's caches (FinetuneGD._forward / _kp_pair are keyed by data_ptr and
belong to the step).  Dataset readers, the random template subsample and PnP (cv2) stay with the caller; TAP-Vid tracking is
not covered.

The reference's own quirks are kept, because the numbers it reports depend on them:
  - the query keypoints of the transfer are sampled with interpolate_features' DEFAULT mapping (patch 14, stride 14) on the
    patch-16 token grid (:542);
  - the target field is the grid upsampled to ds = ((img - p) // s) * s + 1 and edge-padded by p // 2 (:531-538);
  - OnePose++ descriptors are sampled at patch 16 and divided by (norm + 1e-9) (:160-163).
The hard-coded 16 is generalised to the model's patch and stride (equal to the reference's at p = s = 16)."""
import torch

from . import ops
from ._lib import GdHipError


# ----------------------------------------------------------------------------------------------------------------- geometry (host)
def token_grid(img_h, img_w, patch, stride):
    """Token grid of a patch-`patch` / stride-`stride` embedding of an img_h x img_w image: (1 + (img_h - p) // s, 1 + (img_w - p) // s)."""
    if patch <= 0 or stride <= 0 or img_h < patch or img_w < patch:
        raise GdHipError(f"no token grid for image {img_h}x{img_w} at patch {patch}, stride {stride}")
    return 1 + (img_h - patch) // stride, 1 + (img_w - patch) // stride


def transfer_geometry(img_h, img_w, patch, stride):
    """The field of src/evaluate_timm.py:531-538 generalised: -> dict(gh, gw, ds_h, ds_w, top, left, bottom, right).  The grid is
    upsampled to ds = ((img - p) // s) * s + 1 and edge-padded by p // 2 on the top / left and img - ds - p // 2 on the bottom / right."""
    gh, gw = token_grid(img_h, img_w, patch, stride)
    ds_h, ds_w = ((img_h - patch) // stride) * stride + 1, ((img_w - patch) // stride) * stride + 1
    return {"gh": gh, "gw": gw, "ds_h": ds_h, "ds_w": ds_w, "top": patch // 2, "left": patch // 2,
            "bottom": img_h - ds_h - patch // 2, "right": img_w - ds_w - patch // 2}


def keypoint_grid_coords(pts, h, w, patch_size=14, stride=14):
    """interpolate_features' pixel -> grid_sample mapping (utils/functions.py:56-65), in fp32 as the reference computes it:
    pts [..., 2] (x, y) -> [..., 2] in [-1, 1] at the patch centres (7 -> -1 and 623 -> +1 at 640 with the default patch 14)."""
    last_h = ((h - patch_size) // stride) * stride + patch_size / 2
    last_w = ((w - patch_size) // stride) * stride + patch_size / 2
    a = torch.tensor([2 / (last_w - patch_size / 2), 2 / (last_h - patch_size / 2)], dtype=torch.float32, device=pts.device)
    b = torch.tensor([1 - last_w * 2 / (last_w - patch_size / 2), 1 - last_h * 2 / (last_h - patch_size / 2)], dtype=torch.float32,
                     device=pts.device)
    return a * pts.float() + b


def pck(pred_xy, gt_xy, img_size, alphas=(0.10, 0.05, 0.15)):
    """PCK of src/evaluate_timm.py:557-566 on the visible keypoints: fraction with ||pred - gt|| < alpha * img_size, per alpha
    -> fp32 [len(alphas)].  pred_xy int or float [N, 2], gt_xy float [N, 2] (host tensors)."""
    gt = gt_xy.cpu()
    err = (pred_xy.cpu() - gt).norm(dim=-1)
    thr = torch.tensor(alphas) * img_size
    return (err[None, :] < thr[:, None]).sum(dim=-1) / len(gt)


# ----------------------------------------------------------------------------------------------------------------- features
def _backbone(module):
    m = module.model if hasattr(module, "model") else module
    P = m.patch_embed.patch_size[0]
    st = m.patch_embed.proj.stride
    st = (st, st) if isinstance(st, int) else tuple(int(v) for v in st)
    if st[0] != st[1]:
        raise GdHipError(f"correspondence evaluation needs one patch stride, got {st}")
    return m, P, st[0]


def _image(img):
    img = img if img.dim() == 4 else img[None]
    if not (img.is_cuda and img.dtype == torch.float32 and img.shape[1] == 3):
        raise GdHipError("evaluation images are CUDA fp32 [3, H, W] (or [B, 3, H, W]) in [0, 1]")
    return img


def token_maps(module, img):
    """module.model.forward_features on the HIP path, then refine_conv on the whole token grid when the module has one
    (vit.conv3x3_tokens) -> (grid [B, gh * pitch, D] token-major without prefix tokens, gh, gw, pitch)."""
    from .vit import conv3x3_tokens
    m, P, st = _backbone(module)
    img = _image(img)
    H, W = img.shape[-2:]
    gh, gw = token_grid(H, W, P, st)
    with torch.no_grad():
        x = m.forward_features(img)
        prefix = m.num_prefix_tokens
        if x.shape[1] - prefix != gh * gw:
            raise GdHipError(f"the model returned {x.shape[1] - prefix} patch tokens for a {H}x{W} image; patch {P} / stride {st} "
                             f"give a {gh}x{gw} grid")
        rc = getattr(module, "refine_conv", None)
        if rc is not None:
            fmap, pitch = conv3x3_tokens(x, rc.weight, rc.bias, gh, gw)
            return fmap, gh, gw, pitch
        return x[:, prefix:], gh, gw, gw


def _sample(grid, pts, gh, gw, pitch, h, w, patch_size, stride):
    """interpolate_features(normalize=False) on a token-major grid [B, gh * pitch, D] -> [B, N, D] fp32."""
    from .vit import kp_gather
    return kp_gather([grid.contiguous()], pts.float().contiguous(), gh, gw, 1.0, 1.0, h, w, patch_size, stride=stride, pitch=pitch)


def _normalize(x, normalize):
    if normalize is False or normalize is None:
        return x
    if normalize is True:
        return ops.l2_normalize(x.contiguous())                              # F.normalize: x / max(||x||, 1e-12)
    if normalize == "onepose":
        return ops.l2_normalize(x.contiguous(), eps=1e-9)                    # x / (||x|| + 1e-9): the same rows wherever ||x|| >> 1e-9
    raise GdHipError(f"normalize must be True, False or 'onepose', not {normalize!r}")


def descriptors_at(module, img, pts, *, patch_size, stride, normalize):
    """Descriptors of `module` at pixel positions: forward_features (prefix tokens dropped) -> refine_conv on the whole grid if
    the module has one -> interpolate_features(pts, h, w = the image's, patch_size, stride).  img [3, H, W] or [B, 3, H, W]
    in [0, 1]; pts [N, 2] or [B, N, 2] (x, y); normalize True (F.normalize), False, or "onepose" (/(norm + 1e-9)).
    -> [N, D] (or [B, N, D]) fp32."""
    with torch.no_grad():
        single = pts.dim() == 2
        img = _image(img)
        grid, gh, gw, pitch = token_maps(module, img)
        p = pts[None] if single else pts
        if p.shape[0] != grid.shape[0]:
            p = p.expand(grid.shape[0], -1, -1)
        out = _normalize(_sample(grid, p.to(grid.device), gh, gw, pitch, img.shape[-2], img.shape[-1], patch_size, stride), normalize)
        return out[0] if single else out


# ----------------------------------------------------------------------------------------------------------------- OnePose++ matching
def mutual_nearest_neighbours(desc, templates, precision="f16"):
    """The matching block of src/evaluate_timm.py:166-179 from ONE pass of gd_match_argmax: desc [M, D], templates [N, D] ->
    (nbr1 [M] int64 = argmax_j desc_i . t_j, nbr2 [N] int64 = argmax_i desc_i . t_j, mutual [M] bool = nbr2[nbr1] == arange(M)).
    precision "f16" (the reference's TF32 class, fp16 operands under per-tensor power-of-two scales) or "f32" (exact)."""
    with torch.no_grad():
        r = ops.match_argmax(desc, templates, both=True, precision=precision, want_mutual=True)
        return r.row_idx, r.col_idx, r.mutual


# ----------------------------------------------------------------------------------------------------------------- semantic transfer
def _img_hw(img_size):
    return (int(img_size), int(img_size)) if isinstance(img_size, int) else tuple(int(v) for v in img_size)


def transfer_keypoints_from_tokens(tok1, tok2, kps1, img_size=640, patch_size=16, stride=16, query_patch=14, query_stride=14,
                                   pitch=None):
    """kps_1_to_2 of src/evaluate_timm.py:539-547 from the two views' token maps: tok1, tok2 [gh, gw, D] or token-major
    [gh * pitch, D] (after refine_conv when the model has one), gh x gw = 1 + (img - patch) // stride; kps1 [K, >= 2] (x, y, ...).
    The queries are interpolate_features(tok1, kps1, img, img, normalize=True) with the reference's default query mapping
    (query_patch = query_stride = 14); the target field is never materialised: S = q . tok2 on the grid, then the argmax over
    the upsampled, padded S (gd_transfer_argmax).  -> [K, 2] int64 (x, y)."""
    img_h, img_w = _img_hw(img_size)
    gh, gw = token_grid(img_h, img_w, patch_size, stride)
    pitch = gw if pitch is None else int(pitch)
    with torch.no_grad():
        toks = []
        for t in (tok1, tok2):
            t = t.reshape(-1, t.shape[-1])
            if t.shape[0] != gh * pitch:
                raise GdHipError(f"token map of {t.shape[0]} rows; image {img_h}x{img_w} at patch {patch_size}, stride {stride} needs "
                                 f"{gh}x{gw} (pitch {pitch})")
            if not t.is_cuda:
                raise GdHipError("token maps must be CUDA tensors")
            toks.append(t.contiguous() if t.dtype == torch.float32 else ops.cast(t, torch.float32))
        t1, t2 = toks
        K = kps1.shape[0]
        if K == 0:
            return torch.empty(0, 2, dtype=torch.int64, device=t1.device)
        q = _sample(t1[None], kps1[None, :, :2].to(t1.device), gh, gw, pitch, img_h, img_w, query_patch, query_stride)[0]
        q = ops.l2_normalize(q.contiguous())
        S = ops.gemm_nt(q, t2, out_dtype=torch.float32)                    # [K, gh * pitch], exact fp32
        return ops.transfer_argmax(S.view(K, gh, pitch), (img_h, img_w), patch_size, stride)


def transfer_keypoints(module, img1, img2, kps1, img_size=640):
    """The reference's per-pair semantic transfer (src/evaluate_timm.py:509-547) on the HIP path: img1, img2 [3, img, img] fp32 in
    [0, 1] (already resized), kps1 [K, >= 2] (x, y, ...) -> kps_1_to_2 [K, 2] int64 (x, y) in view 2."""
    img_h, img_w = _img_hw(img_size)
    for im in (img1, img2):
        if tuple(im.shape[-2:]) != (img_h, img_w):
            raise GdHipError(f"image {tuple(im.shape[-2:])} is not img_size {(img_h, img_w)}")
    _, P, st = _backbone(module)
    g1, gh, gw, pitch = token_maps(module, img1)
    g2, _, _, _ = token_maps(module, img2)
    return transfer_keypoints_from_tokens(g1[0], g2[0], kps1, (img_h, img_w), P, st, pitch=pitch)


def semantic_transfer_pck(module, pairs, img_size=640, alphas=(0.10, 0.05, 0.15)):
    """PCK-Transfer of src/evaluate_timm.py:461-566 over already-loaded pairs (img1, img2, kps1, kps2): kps [K, 3] (x, y, visibility),
    images as `transfer_keypoints` takes them.  The visible keypoints (v1 * v2 > 0) of all pairs are pooled, as the reference pools
    a category -> {"PCK0.10": ..., ...} in `alphas` order, plus "n" (pooled keypoints)."""
    preds, gts = [], []
    for img1, img2, kps1, kps2 in pairs:
        xy = transfer_keypoints(module, img1, img2, kps1, img_size).cpu()
        k2 = kps2.cpu()
        vis = kps1[:, 2].cpu() * k2[:, 2] > 0
        gts.append(k2[vis][:, [1, 0]])
        preds.append(xy[vis][:, [1, 0]])
    if not gts or sum(len(g) for g in gts) == 0:
        raise GdHipError("semantic_transfer_pck: no visible keypoints")
    res = pck(torch.cat(preds), torch.cat(gts), img_size if isinstance(img_size, int) else max(_img_hw(img_size)), alphas)
    out = {f"PCK{a:.2f}": float(v) for a, v in zip(alphas, res.tolist())}
    out["n"] = int(sum(len(g) for g in gts))
    return out
